"""The cycle loops of a 3x3-only 8-lane plan kernel, counted from its gfx950 assembly (no GPU needed).

    hipcc <the flags of quadrupedal_foothold_planner_amd/build.py without -shared -fPIC> --cuda-device-only -S \
        -x hip quadrupedal_foothold_planner_amd/csrc/fpe_kernels.hip -o fpe_kernels.s
    python3 profiles/hot_cycle_listing.py fpe_kernels.s ['plan_bits_kernel<2, true, 2>'] [--listing]

Loops are taken from the compiler's own block comments ("in Loop: Header=BBf_n Depth=d", "This Loop Header").  A cycle loop is a
loop whose OWN blocks (not a child loop's) hold the elevation row load of leg_fast8m (global_load_dwordx3: once per copy of the body
in the instances with two and three window rows per lane): the plain copy's at depth 2 (batch, cycle), the general copy's at depth 3
(batch, cycle, phase).  Its SPAN is the contiguous run of its own blocks around the header; own blocks laid out elsewhere, and the
child loops (the general leg search and the candidate search beyond rank 15 have loops), are the cold bodies.  With branch weights
on the rare guards (FPE_RARE) the span is the executed path of a cycle that takes no rare branch, top to bottom; instructions
between a forward s_cbranch_execz and its target inside the span run only while some lane is active there (the candidate search
behind !defaultOk, the stores of lane 0) and are counted apart, "guarded".
Stages are cut, in the span's order, behind the instruction that ends them: see STAGES.
"""
import re
import subprocess
import sys
from collections import Counter

LOAD = "global_load_dwordx3"
CLASSES = ["valu", "valu_f64", "salu", "lds", "vmem", "smem", "branch", "s_waitcnt", "s_nop", "v_readlane", "v_writelane", "other"]
# (name, the mnemonic that ends the stage, which occurrence counted from the stage's start; 0: the last one in the span;
# "@search": the end of the span's largest guarded region, the candidate search behind !defaultOk)
STAGES = [("feet-polygon centre: LDS reads, division", "v_div_fixup_f64", 1),
          ("div3, x pass, indices by DPP, window request", "global_load_dwordx4", 0),
          ("boxes, rare verdict, submap, elevation row load", LOAD, 1),
          ("membership, window rows, default check, deposits, centroid selects, search", "@search", 0),
          ("unit record, commit, validation ballot, loop end", None, 0)]


def kernel_body(lines, want):
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if not m:
            continue
        dn = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout
        if want in dn.replace("(anonymous namespace)::", ""):
            for j in range(i, len(lines)):
                if lines[j].startswith(".Lfunc_end"):
                    return i, j
    raise SystemExit(f"no kernel matching {want!r}")


def classify(mn):
    if mn.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    for k in ("s_waitcnt", "s_nop", "v_writelane"):
        if mn.startswith(k):
            return k
    if mn.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if mn.startswith(("v_readlane", "v_readfirstlane")):
        return "v_readlane"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if mn.startswith("v_"):
        return "valu_f64" if "f64" in mn else "valu"
    return "salu" if mn.startswith("s_") else "other"


def parse(lines, a, b):
    """Blocks of lines[a:b] in layout order: dict(label, loop = innermost loop's header label or None, depth, ins = [(line, mnemonic, operands)])."""
    blocks, parents = [], {}
    cur = dict(label="entry", loop=None, depth=0, ins=[])
    blocks.append(cur)
    n = a + 1
    while n < b:
        l = lines[n]
        m = re.match(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)(.*)", l)
        if m:
            label, rest = m.group(1), m.group(2)
            notes = [rest]
            while n + 1 < b and re.match(r"^\s+;", lines[n + 1]) and not re.match(r"^\s+; (implicit-def|kill)", lines[n + 1]):
                n += 1
                notes.append(lines[n])
            note = "\n".join(notes)
            loop, depth = None, 0
            mi = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            mh = re.search(r"This Loop Header: Depth=(\d+)", note)
            if mh and label:
                loop, depth = label[2:], int(mh.group(1))
                ps = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", note)
                parents[loop] = ps[-1][0] if ps else None
            elif mi:
                loop, depth = mi.group(1), int(mi.group(2))
            cur = dict(label=label or "", loop=loop, depth=depth, ins=[])
            blocks.append(cur)
        else:
            m = re.match(r"^\t([a-z_0-9]+)\s*([^;]*)", l)
            if m and not l.startswith("\t."):
                cur["ins"].append((n + 1, m.group(1), m.group(2).strip()))
        n += 1
    return blocks, parents


def counts(ins):
    return Counter(classify(mn) for _, mn, _ in ins)


def row(name, c, g=None):
    cells = " ".join((f"{c[k]:5d}" + (f"|{g[k]:<4d}" if g is not None else "")) for k in CLASSES)
    tot = f"{sum(c.values()):5d}" + (f"|{sum(g.values()):<4d}" if g is not None else "")
    return f"  {name:76s} {tot}  {cells}"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lines = open(args[0]).read().splitlines()
    want = args[1] if len(args) > 1 else "plan_bits_kernel<2, true, 2>"
    a, b = kernel_body(lines, want)
    blocks, parents = parse(lines, a, b)
    total = sum(len(bl["ins"]) for bl in blocks)
    print(f"{want}: {total} instructions, {len(parents)} loops")
    heads = sorted({(bl["depth"], bl["loop"]) for bl in blocks if bl["loop"] and any(mn == LOAD for _, mn, _ in bl["ins"])})
    hdr = " " * 79 + "total  " + " ".join(f"{k[:9]:>9s}" if False else f"{k[:5]:>5s}" for k in CLASSES)
    for depth, head in heads:
        def inside(lp):
            while lp:
                if lp == head:
                    return True
                lp = parents.get(lp)
            return False
        own = [i for i, bl in enumerate(blocks) if bl["loop"] == head]
        hi = next(i for i in own if blocks[i]["label"] == ".L" + head)
        lo = hi
        while lo - 1 in own:
            lo -= 1
        up = hi
        while up + 1 in own:
            up += 1
        span = [x for i in range(lo, up + 1) for x in blocks[i]["ins"]]
        # ... which ends at the loop's last backward branch to the header or to an own block laid out in front of it (a rotated
        # loop's end): own blocks behind it are cold bodies that were placed next to the loop and jump back into it
        early, k = set(), 0
        for i in range(lo, up + 1):
            if i <= hi and blocks[i]["label"]:
                early.add(blocks[i]["label"])
            k += len(blocks[i]["ins"])
        back = [i for i, (_, mn, ops) in enumerate(span) if mn.startswith(("s_cbranch", "s_branch")) and ops in early]
        tail = span[back[-1] + 1:] if back else []
        span = span[:back[-1] + 1] if back else span
        cold_own = tail + [x for i in own if not lo <= i <= up for x in blocks[i]["ins"]]
        child = [x for bl in blocks if bl["loop"] != head and inside(bl["loop"]) for x in bl["ins"]]
        first_line = min(x[0] for i, bl in enumerate(blocks) if inside(bl["loop"]) for x in bl["ins"])
        last_line = max(x[0] for i, bl in enumerate(blocks) if inside(bl["loop"]) for x in bl["ins"])
        between = [x for bl in blocks for x in bl["ins"] if first_line <= x[0] <= last_line]
        kind = "plain copy" if depth == heads[0][0] and len(heads) > 1 else ("general copy" if len(heads) > 1 else "only copy found")
        print(f"\ncycle loop {head} (depth {depth}: {kind})")
        print(f"  the loop with its cold bodies lies in lines {first_line}..{last_line} ({len(between)} instructions of any block laid out there)")
        print(hdr)
        print(row(f"span around the header, lines {span[0][0]}..{span[-1][0]}", counts(span)))
        print(row("own blocks laid out elsewhere (cold bodies without loops)", counts(cold_own)))
        print(row("child loops (cold bodies with loops)", counts(child)))
        cb = sum(1 for _, mn, _ in span if mn.startswith("s_cbranch"))
        ub = sum(1 for _, mn, _ in span if mn.startswith("s_branch"))
        print(f"  span: {cb} conditional and {ub} unconditional branches")
        if depth != heads[0][0]:
            continue
        # stages of the span; guarded = between a forward s_cbranch_execz and its target inside the span
        pos = {}
        k = 0
        for i in range(lo, up + 1):
            if blocks[i]["label"]:
                pos[blocks[i]["label"]] = k
            k += len(blocks[i]["ins"])
        guarded = [False] * len(span)
        for i, (_, mn, ops) in enumerate(span):
            if mn == "s_cbranch_execz" and ops in pos and pos[ops] > i:
                for j in range(i + 1, min(pos[ops], len(span))):
                    guarded[j] = True
        cuts, start = [], 0
        for name, key, occ in STAGES:
            if key is None:
                end = len(span)
            elif key == "@search":
                best, i = (0, start), 0
                while i < len(span):
                    j = i
                    while j < len(span) and guarded[j]:
                        j += 1
                    best = max(best, (j - i, j))
                    i = j + 1
                end = max(best[1], start)
            else:
                hits = [i for i in range(start, len(span)) if span[i][1] == key]
                end = (hits[-1] if occ == 0 else hits[occ - 1]) + 1 if hits else start
            cuts.append((name, start, end))
            start = end
        print(f"\n  stages of the span, straight|guarded (guarded: under a forward s_cbranch_execz, executed while a lane is active there)")
        print(hdr)
        for name, s, e in cuts:
            st = counts([span[i] for i in range(s, e) if not guarded[i]])
            gd = counts([span[i] for i in range(s, e) if guarded[i]])
            print(row(name, st, gd))
        st = counts([x for x, g in zip(span, guarded) if not g])
        gd = counts([x for x, g in zip(span, guarded) if g])
        print(row("whole span", st, gd))
        runs, i = [], 0
        while i < len(span):
            if guarded[i]:
                j = i
                while j < len(span) and guarded[j]:
                    j += 1
                runs.append((span[i][0], j - i))
                i = j
            else:
                i += 1
        print("  guarded regions (first line: instructions): " + ", ".join(f"{ln}: {n}" for ln, n in runs))
        if "--listing" in sys.argv:
            for (ln, _, _), g in zip(span, guarded):
                print(("  ~ " if g else "    ") + lines[ln - 1].strip())


if __name__ == "__main__":
    main()
