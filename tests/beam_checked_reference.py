"""The reference of the checked beam (fpe_plan_beam_checked*; include/fpe.h, "checked beam"): the header's semantics in
plain Python.  The loop is tests/beam_reference.beam's — resume_reference.resume_pose for the chains, segment_penalty for q,
candidate_score for the progress term.  No check arithmetic is restated: the path summaries of a candidate are
rank_checked_reference.summaries on the candidate's concatenated path so far, from the root's start feet, and the fold is
rank_checked_reference.fold's chain on P_c.  What this file adds: the carried feet (from the products), the class rule on the final
score and the bookkeeping.  A helper, not a test: tests/test_cpu_beam_checked.py pins it and asserts what the GPU tests' inputs must
exercise; tests/test_gpu_beam_checked.py compares the engine with it.  Each reference is computed once per process (the callers must
not write into what they get)."""
import functools
import math

import numpy as np

from oracle import fpo
from quadrupedal_foothold_planner_amd import _capi
from tests import beam_reference as bref
from tests import margin_reference, swing_reference
from tests import rank_checked_reference as cref
from tests import resume_reference as rref

SUMS = {"swing": (cref.SWING, _capi.SWING_SUMMARY_DTYPE), "trunk": (cref.TRUNK, _capi.TRUNK_SUMMARY_DTYPE),
        "margin": (cref.MARGIN, _capi.MARGIN_SUMMARY_DTYPE)}
FREE = dict(checks=7, reject=0, w_swing_over=0.0, w_lift=0.0, w_trunk_bad=0.0, w_margin_under=0.0, w_unknown=0.0, swing=None,
            trunk=dict(ride_height=cref.RIDE_HEIGHT), margin=cref.MARGIN_LIMIT)   # no limit acts, no term weighs: the unchecked order


def environment(c):
    """What the summaries need of a case (beam_reference.case): the map, the margin's thresholds, the foot radius and the body"""
    p = c["params"]
    return dict(omap=fpo.OracleMap(c["trav"], c["elev"], c["row"].res), trav=c["trav"], elev=c["elev"], res=c["row"].res,
                thr=margin_reference.thresholds(p), foot_radius=float(p["footRadius"][0]),
                body=(np.float32(p["length"][0]), np.float32(p["width"][0])), oparams=c["oparams"])


def path_summaries(env, nominal, cycle_ok, start_feet, checks):
    """The summaries of the enabled checks over whole paths: nominal [n, cycles, 4], cycle_ok [n, cycles], start_feet [n, 4, 3]"""
    return cref.summaries(env["trav"], env["elev"], env["res"], (0.0, 0.0), env["thr"], nominal, cycle_ok, start_feet, checks,
                          env["foot_radius"], env["body"])


def carried_feet(nominal, cycle_ok, start_feet):
    """Per leg (x, y, double(z)) of the nominal record of the latest committed cycle of a path, else the start feet: [4, 3]"""
    feet = np.array(start_feet, dtype=np.float64).reshape(4, 3)
    done = np.nonzero(cycle_ok)[0]
    if done.size:
        g = int(done[-1])
        feet = np.stack([nominal["x"][g], nominal["y"][g], nominal["z"][g].astype(np.float64)], axis=1)
    return feet


def stance_of(env, oposes):
    """The `stance` product of the roots' plans (the same for every stride option): the start feet of a call without start_feet"""
    return env["omap"].plan(env["oparams"], oposes, 1)["stance"]


def ground_feet(env, stance):
    """The explicit start feet of the cases: the stance's x, y with z the elevation of the foot's cell, 0 where that cell is unknown
    or off the map"""
    grid = swing_reference.Grid(env["elev"], env["res"])
    feet = np.array(stance, dtype=np.float64)
    for idx in np.ndindex(feet.shape[:-1]):
        x, y = feet[idx][0], feet[idx][1]
        z = 0.0
        if grid.within(x, 0) and grid.within(y, 1):
            r, col = int(np.argmin(np.abs(grid.px[:, 0] - x))), int(np.argmin(np.abs(grid.py[0, :] - y)))
            z = float(grid.elev[r, col]) if grid.known[r, col] else 0.0
        feet[idx][2] = z
    return feet


def beam(env, poses, options, S, k, W, weights, checks, start_feet, states=None, segment_sums=False):
    """The checked beam of every root (poses in the oracle's layout; start_feet [B, 4, 3]: given, or the stance).  Returns
    beam_reference.beam's dict — "penalty" holds v — plus "base_penalty", "hit" [B, n], "feet" [B, n, 4, 3], "sums": {check: [B, n]
    summaries} of the enabled checks, and in "log" per root and segment every candidate's score, class, hit, base penalty, committed
    cycles, carried feet, the path summaries, the survivors, and "unchecked": what the unchecked order keeps from the same candidates
    (segment_sums: also "segment", the summaries of the candidate's own k cycles from its parent's feet)."""
    ck = cref.check_params(checks)
    on, reject = int(ck["checks"]), int(ck["reject"])
    B, M = poses.shape[0], options.shape[0]
    n_final = min(W, M ** S)
    res = {"n_live": np.full(B, n_final, np.int32), "path": np.zeros((B, n_final, S), np.uint8), "score": np.zeros((B, n_final)),
           "penalty": np.zeros((B, n_final)), "base_penalty": np.zeros((B, n_final)), "hit": np.zeros((B, n_final), np.uint8),
           "feet": np.zeros((B, n_final, 4, 3)), "state": np.zeros((B, n_final), rref.STATE_DTYPE), "log": [],
           "sums": {q: np.zeros((B, n_final), dt) for q, (bit, dt) in SUMS.items() if on & bit},
           "cycle0": np.array([0 if states is None else int(states[b]["cycle"]) for b in range(B)])}
    plans = []
    for b in range(B):
        root_feet = np.array(start_feet[b], dtype=np.float64).reshape(4, 3)
        entries = [dict(base=0.0, state=None if states is None else states[b], path=(), segs=(), feet=root_feet)]
        log = []
        for s in range(S):
            cands = []
            for p, e in enumerate(entries):
                for m in range(M):
                    start = e["state"] if e["state"] is not None else rref.state_from_pose(env["oparams"], poses[b], options[m])
                    plan, sts = rref.resume_pose(env["omap"], env["oparams"], poses[b], start, k, options[m])
                    cands.append(dict(c=p * M + m, base=e["base"] + bref.segment_penalty(plan, k, weights), state=sts[-1],
                                      path=e["path"] + (m,), segs=e["segs"] + (plan,), parent_feet=e["feet"],
                                      committed=int(np.count_nonzero(plan["cycle_ok"]))))
            nominal = np.stack([np.concatenate([sg["nominal"] for sg in q["segs"]]) for q in cands])
            cycle_ok = np.stack([np.concatenate([sg["cycle_ok"] for sg in q["segs"]]) for q in cands])
            sums = path_summaries(env, nominal, cycle_ok, np.broadcast_to(root_feet, (len(cands), 4, 3)), ck) if on else {}
            fold = cref.fold(np.array([q["base"] for q in cands]), np.zeros(len(cands)), sums, ck)
            for i, q in enumerate(cands):
                q["v"], q["hit"] = float(fold["score"][i]), int(fold["hit"][i])
                q["score"] = bref.candidate_score(q["v"], q["state"], weights)[0]
                q["cls"] = 2 if not math.isfinite(q["score"]) else (1 if q["hit"] & reject else 0)
                q["feet"] = carried_feet(nominal[i], cycle_ok[i], root_feet)
                q["sums"] = {name: sums[name][i] for name in sums}
                plain = bref.candidate_score(q["base"], q["state"], weights)
                q["plain"] = (plain[1], plain[0] if plain[1] == 0 else 0.0, q["c"])
            order = sorted(cands, key=lambda q: (q["cls"], q["score"] if q["cls"] < 2 else 0.0, q["c"]))
            keep = order[:min(W, len(cands))]
            entry = {"scores": [q["score"] for q in cands], "classes": [q["cls"] for q in cands], "hits": [q["hit"] for q in cands],
                     "base": [q["base"] for q in cands], "committed": [q["committed"] for q in cands],
                     "feet": [q["feet"] for q in cands], "parent_feet": [q["parent_feet"] for q in cands],
                     "sums": {name: sums[name] for name in sums}, "survivors": [q["c"] for q in keep],
                     "unchecked": [q["c"] for q in sorted(cands, key=lambda q: q["plain"])[:len(keep)]]}
            if segment_sums:
                entry["segment"] = path_summaries(env, nominal[:, s * k:], cycle_ok[:, s * k:], np.stack([q["parent_feet"] for q in cands]), ck)
            log.append(entry)
            entries = [dict(base=q["base"], state=q["state"], path=q["path"], segs=q["segs"], feet=q["feet"], final=q) for q in keep]
        assert len(entries) == n_final
        for w, e in enumerate(entries):
            q = e["final"]
            res["path"][b, w], res["score"][b, w], res["penalty"][b, w], res["state"][b, w] = q["path"], q["score"], q["v"], q["state"]
            res["base_penalty"][b, w], res["hit"][b, w], res["feet"][b, w] = q["base"], q["hit"], q["feet"]
            for name in res["sums"]:
                res["sums"][name][b, w] = q["sums"][name]
        plans.append([{key: np.concatenate([sg[key] for sg in e["segs"]]) for key in bref.PLAN_KEYS} for e in entries])
        res["log"].append(log)
    res["plan"] = {key: np.stack([np.stack([slot[key] for slot in root]) for root in plans]) for key in bref.PLAN_KEYS}
    return res


# ---- the inputs of tests/test_gpu_beam_checked.py (their conditions are asserted on this helper alone in tests/test_cpu_beam_checked.py)
# the rows and shapes of beam_reference.CASES; "stance_start": w16_seq with start_feet NULL — the roots start from the plan's stance;
# "w48_raised": w48_direct with the start feet a centimetre above the ground (a sole): with the feet AT ground height the lowest path
# max_lift of any case is +0.0011, a centimetre higher the chords of root 1's first swings pass over everything under them and three
# final slots hold max_lift = -0.0056
CASES = ("w7_gen", "w7_gen_k5", "w16_seq", "w48_direct", "underfilled", "resumed", "largest_sort", "nan_option", "stance_start", "w48_raised")
ALIAS = {"stance_start": "w16_seq", "w48_raised": "w48_direct"}
WEIGHTS = dict(w_swing_over=7.0, w_lift=40.0, w_trunk_bad=9.0, w_margin_under=3.0, w_unknown=2.0)
REJECT = cref.SWING | cref.TRUNK


def base_case(name):
    return bref.case(ALIAS.get(name, name))


@functools.lru_cache(maxsize=None)
def start_feet(name):
    """[B, 4, 3]: the ground-height feet under the stance (resumed roots: under the state's nominal track); for "stance_start" the
    stance itself (what a NULL start_feet means); for "w48_raised" a centimetre above the ground"""
    c = base_case(name)
    env = environment(c)
    stance = stance_of(env, c["oroots"])
    if c["states"] is not None:  # resumed roots: where the nominal track's feet stand
        stance = stance.copy()
        stance[:, :, :2] = c["states"]["feet"][:, 2]
    if name == "stance_start":
        return stance
    feet = ground_feet(env, stance)
    if name == "w48_raised":
        feet[..., 2] += 0.01
    return feet


@functools.lru_cache(maxsize=None)
def free_reference(name):
    """The case with no limit and no weight: the unchecked beam's candidates, with every candidate's own segment summarised"""
    c = base_case(name)
    return beam(environment(c), c["oroots"], c["options"], c["S"], c["k"], c["W"], c["weights"], FREE, start_feet(name), c["states"],
                segment_sums=True)


@functools.lru_cache(maxsize=None)
def limits(name):
    """The limits of a case, derived from its data as rank_checked_reference.derived_limits does: max_lift and min_clearance are the
    medians of the free per-candidate values (one segment each, from the parent's feet) over all candidates of the unchecked beam's
    segments; ride_height 0.25; the margin block rank_checked_reference.MARGIN_LIMIT."""
    segs = [sg["segment"] for root in free_reference(name)["log"] for sg in root]
    lift = np.concatenate([sg["swing"]["max_lift"][sg["swing"]["n_segments"] > 0] for sg in segs])
    clear = np.concatenate([sg["trunk"]["min_clearance"][np.isfinite(sg["trunk"]["min_clearance"])] for sg in segs])
    return dict(swing=dict(max_lift=float(np.median(lift))), trunk=dict(ride_height=cref.RIDE_HEIGHT, min_clearance=float(np.median(clear))),
                margin=dict(cref.MARGIN_LIMIT))


def checks_of(name, **over):
    """The checks dict (rank_checked_reference.check_params' keys) of a case: all three checks, the derived limits, WEIGHTS, REJECT"""
    ck = dict(limits(name), checks=7, reject=REJECT, **WEIGHTS)
    ck.update(over)
    return ck


def run(name, checks, feet=None, states="case"):
    c = base_case(name)
    return beam(environment(c), c["oroots"], c["options"], c["S"], c["k"], c["W"], c["weights"], checks,
                start_feet(name) if feet is None else feet, c["states"] if isinstance(states, str) else states)


@functools.lru_cache(maxsize=None)
def reference(name):
    return run(name, checks_of(name))


def conditions(ref, k):
    """What a case's inputs exercise, from a beam() result alone"""
    segs = [sg for root in ref["log"] for sg in root]
    hit = ref["hit"].reshape(-1)
    ties = False
    for sg in segs:  # an exact tie between two candidates of one class where one survives
        kept = set(sg["survivors"])
        finite = [(cl, sc, c) for c, (sc, cl) in enumerate(zip(sg["scores"], sg["classes"])) if cl < 2]
        for cl, sc, c in finite:
            ties = ties or any(sc == sc2 and cl == cl2 and c != c2 and (c in kept or c2 in kept) for cl2, sc2, c2 in finite)
    inherits = False
    for root in ref["log"]:  # a candidate that commits nothing keeps its parent's feet; a child of it starts its first swing there
        for s, sg in enumerate(root[:-1]):
            for c, n in enumerate(sg["committed"]):
                if n == 0 and c in sg["survivors"] and np.array_equal(sg["feet"][c], sg["parent_feet"][c]):
                    w = sg["survivors"].index(c)
                    nxt = root[s + 1]
                    M = len(nxt["committed"]) // len(sg["survivors"])
                    inherits = inherits or any(nxt["committed"][w * M + m] > 0 and np.array_equal(nxt["parent_feet"][w * M + m], sg["feet"][c])
                                               for m in range(M))
    sums = ref["sums"]
    firsts = []
    if "swing" in sums:
        firsts += sums["swing"]["first_over_cycle"].reshape(-1).tolist() + [int(v) for v in sums["margin"]["first_under_cycle"].reshape(-1)] \
            + sums["trunk"]["first_bad_cycle"].reshape(-1).tolist()
    return {
        "checked_survivors_differ_from_the_unchecked": any(sg["survivors"] != sg["unchecked"] for sg in segs),
        "class_0_and_class_1_in_one_segment": any({0, 1} <= set(sg["classes"]) for sg in segs),
        "only_class_1_and_still_full_in_score_order": any(
            set(sg["classes"]) == {1} and len(sg["survivors"]) > 1
            and [sg["scores"][c] for c in sg["survivors"]] == sorted(sg["scores"][c] for c in sg["survivors"]) for sg in segs),
        "every_hit_bit_set_and_clear": all(0 < np.count_nonzero(hit & bit) < hit.size for bit in (1, 2, 4, 8)),
        "a_candidate_without_commits_inherits_its_parents_feet": inherits,
        "a_negative_max_lift": any(bool(((sg["sums"]["swing"]["max_lift"] < 0) & (sg["sums"]["swing"]["n_segments"] > 0)).any())
                                   for sg in segs if "swing" in sg["sums"]),
        "a_global_first_cycle": any(k <= v < 255 for v in firsts),
        "an_exact_tie_at_a_survivor": ties,
    }
