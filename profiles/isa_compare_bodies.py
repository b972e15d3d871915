"""Compare the device code of two builds, symbol by symbol: isa_compare_bodies.py BASE.s HEAD.s [symbol expected to leave | OLD=NEW ...]

BASE.s / HEAD.s: csrc/fpe_kernels.hip compiled with build.py's FLAGS minus -shared, plus --offload-device-only -S.
Every kernel (.amdhsa_kernel) and every device function (@function) is cut from `<symbol>:` to its `.Lfunc_end`, the
function-numbered local labels (.LBB<n>_, .Ltmp<n>, .Lfunc_begin<n>) are renumbered away, and the texts are compared; the kernels'
metadata lines (isa_kernel_metadata.py) are compared as well.  A host-side change leaves every common body identical and the
symbol sets equal but for what it names as leaving (substrings of demangled names).  Exit status 1 otherwise.

OLD=NEW pairs a kernel of BASE with the kernel of HEAD that replaces it under another name (both as isa_kernel_metadata.py prints
them, without the namespace: "plan_sequential_stride_kernel=plan_sequential_kernel<fpe_stride const*>").  The pair is compared as one
common symbol, body and metadata line, with HEAD's symbol name rewritten to BASE's.

One difference follows from a kernel leaving or joining and is accepted only when proved harmless: a kernel that calls a device
function which uses dynamic LDS passes its ordinal among such kernels in s15 (`s_mov_b32 s15, <id>`), the callee's index into
llvm.amdgcn.dynlds.offset.table.  Removing a kernel renumbers the ones behind it.  Bodies that differ in these immediates only are
listed on their own, and pass when the renumbering keeps the order and every kernel reads the same table entry as before.
"""
import collections
import os
import re
import subprocess
import sys


def bodies(path):
    text = open(path).read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out = {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n", text, re.M):
        sym = m.group(1)
        start = text.index("\n" + sym + ":", m.end() - 1)
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, start).start()
        body = text[start:end]
        body = re.sub(r"((?:\.L|\b)BB)\d+_", r"\1_", body)  # labels (.LBB<n>_<k>) and the loop comments that name them (BB<n>_<k>)
        body = re.sub(r"\.L(tmp|func_begin)\d+", r".L\1", body)
        body = re.sub(r"[ \t]+;", " ;", body)  # (comment columns move with the width of a label)
        body = re.sub(r"^\t\.section\t\.text\.\S+$", "\t.text", body, flags=re.M)  # (a template's kernel descriptor sits in its own section)
        out[sym] = body
    assert kernels <= set(out), sorted(kernels - set(out))
    return kernels, out


LDS_ID = re.compile(r"^\ts_mov_b32 s15, (\d+)$", re.M)


def dynlds_table(path):
    m = re.search(r"^llvm\.amdgcn\.dynlds\.offset\.table:\n((?:\t\.long\t\S+\n)*)", open(path).read(), re.M)
    return re.findall(r"\.long\t(\S+)", m.group(1)) if m else []


def metadata(path):
    tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa_kernel_metadata.py")
    return collections.Counter(subprocess.run([sys.executable, tool, path], capture_output=True, text=True, check=True).stdout.splitlines())


def demangle(syms):
    syms = sorted(syms)
    return subprocess.run(["c++filt"] + syms, capture_output=True, text=True).stdout.splitlines() if syms else []


def short(name):
    """A demangled kernel name as isa_kernel_metadata.py prints it, without the namespace."""
    name = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "").replace("void fpe::", ""))
    return name[5:] if name.startswith("fpe::") else name


def renamed_line(line, names):
    name = short(line[:80].strip())
    return f"{names.get(name, name):80s}" + line[80:]


def main():
    base, head = sys.argv[1], sys.argv[2]
    leaving = [a for a in sys.argv[3:] if "=" not in a]
    pairs = dict(a.split("=", 1) for a in sys.argv[3:] if "=" in a)
    (kb, fb), (kh, fh) = bodies(base), bodies(head)
    print(f"base: {len(kb)} kernels, {len(fb) - len(kb)} device functions; head: {len(kh)} kernels, {len(fh) - len(kh)} device functions")
    only_b, only_h = sorted(set(fb) - set(fh)), sorted(set(fh) - set(fb))
    by_short_b, by_short_h = dict(zip(map(short, demangle(only_b)), only_b)), dict(zip(map(short, demangle(only_h)), only_h))
    for old, new in pairs.items():
        so, sn = by_short_b[old], by_short_h[new]  # (KeyError: no such kernel on that side)
        fh[so] = fh.pop(sn).replace(sn, so)
        if sn in kh:
            kh = (kh - {sn}) | {so}
        print("paired:", old, "=", new)
    gone, new = demangle(set(fb) - set(fh)), demangle(set(fh) - set(fb))
    for name in gone:
        print("only in base:", name)
    for name in new:
        print("only in head:", name)
    changed = [s for s in set(fb) & set(fh) if fb[s] != fh[s]]
    ids_only = [s for s in changed if LDS_ID.sub("\ts_mov_b32 s15, <id>", fb[s]) == LDS_ID.sub("\ts_mov_b32 s15, <id>", fh[s])]
    differ = demangle(set(changed) - set(ids_only))
    for name in differ:
        print("body differs:", name)
    print(f"{len(set(fb) & set(fh))} common symbols, {len(differ)} with a different body")
    if not ids_only:
        print("llvm.amdgcn.dynlds.offset.table:", "identical" if dynlds_table(base) == dynlds_table(head) else "DIFFERS", f"({len(dynlds_table(head))} entries)")
    renumber = sorted({(int(a), int(b)) for s in ids_only for a, b in zip(LDS_ID.findall(fb[s]), LDS_ID.findall(fh[s]))})
    tb, th = dynlds_table(base), dynlds_table(head)
    ids_ok = all(a1 < a2 and b1 < b2 for (a1, b1), (a2, b2) in zip(renumber, renumber[1:])) and all(tb[a] == th[b] for a, b in renumber)
    if ids_only:
        print(f"{len(ids_only)} kernels differ in their dynamic-LDS kernel id (s15) only; base id -> head id:", " ".join(f"{a}->{b}" for a, b in renumber))
        print(f"  llvm.amdgcn.dynlds.offset.table: {len(tb)} entries -> {len(th)};",
              "order kept, every kernel reads the entry it read before" if ids_ok else "NOT a harmless renumbering")
    back = {new[:80]: old for old, new in pairs.items()}
    mb = collections.Counter(renamed_line(line, {}) for line in metadata(base).elements())
    mh = collections.Counter(renamed_line(line, back) for line in metadata(head).elements())
    for line in sorted((mb - mh).elements()):
        print("metadata only in base:", line)
    for line in sorted((mh - mb).elements()):
        print("metadata only in head:", line)
    unexpected = [n for n in gone if not any(w in n for w in leaving)]
    ok = not new and not differ and ids_ok and not unexpected and not (mh - mb) and sum((mb - mh).values()) == len(set(kb) - set(kh))
    print("device code unchanged" + (f" but for {len(gone)} symbols that left" if gone else "") if ok else "DEVICE CODE CHANGED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
