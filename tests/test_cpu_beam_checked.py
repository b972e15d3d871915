"""The checked beam (fpe_plan_beam_checked*; include/fpe.h) without a GPU: the C side of the new ABI, the reference helper
(tests/beam_checked_reference.py) against the unchecked beam's helper, against brute force and against the checks' own references, and
the conditions the GPU tests' inputs have to meet — asserted on the helper alone, so that the GPU cases cannot be hollow."""
import ctypes as C
import itertools

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from tests import abi_c
from tests import beam_checked_reference as bcref
from tests import beam_reference as bref
from tests import rank_checked_reference as cref
from tests import resume_reference as rref

C_PROTOTYPES = {
    "fpe_plan_beam_checked": "int (*)(fpe_handle, const fpe_params*, const fpe_beam_params*, const fpe_check_params*, const fpe_pose*, "
                             "const fpe_plan_state*, const double*, int32_t, const fpe_stride*, int32_t, const fpe_beam_out*, "
                             "const fpe_beam_check_out*)",
    "fpe_plan_beam_checked_device": "int (*)(fpe_handle, const fpe_params*, const fpe_beam_params*, const fpe_check_params*, const fpe_pose*, "
                                    "const fpe_plan_state*, const double*, int32_t, const fpe_stride*, int32_t, const fpe_beam_out*, "
                                    "const fpe_beam_check_out*, void*)",
}


def test_checked_beam_abi_is_plain_c_and_leaves_the_version_alone(tmp_path):
    """fpe_beam_check_out is six pointers, both entry points assign to plain-C function pointers under warnings as errors,
    FPE_ABI_VERSION still prints 5, the older structs keep their sizes, and the new symbols are in the binding's table and the library."""
    decls = "".join(f"  {proto.replace('(*)', f'(*p{k})')} = {name}; (void)p{k};\n" for k, (name, proto) in enumerate(C_PROTOTYPES.items()))
    body = ("  fpe_beam_check_out co; co.feet = 0; (void)co;\n"
            '  printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(fpe_beam_check_out), offsetof(fpe_beam_check_out, base_penalty), '
            "offsetof(fpe_beam_check_out, feet), sizeof(fpe_beam_out), sizeof(fpe_check_params), sizeof(fpe_check_out), FPE_ABI_VERSION);")
    assert abi_c.compile_and_run(tmp_path, body, decls).split() == ["48", "24", "40", "104", "160", "40", "5"]
    assert C.sizeof(_capi.BeamCheckOut) == 48 and _capi.STRUCTS["fpe_beam_check_out"] is _capi.BeamCheckOut and _capi.ABI_VERSION == 5
    assert [f for f, _ in _capi.BeamCheckOut._fields_] == ["swing", "trunk", "margin", "base_penalty", "hit", "feet"]
    L = _capi.lib()
    for name in C_PROTOTYPES:
        assert name in _capi.PROTOTYPES and hasattr(L, name), name
    cp = _capi.CheckParams()
    assert L.fpe_check_params_defaults(C.byref(cp)) == _capi.FPE_OK   # the defaults a NULL `checks` means: those of the checked ranking
    assert (cp.checks, cp.reject, cp.w_swing_over, cp.w_lift, cp.w_trunk_bad, cp.w_margin_under, cp.w_unknown) == (7, 0, 10.0, 0.0, 10.0, 1.0, 1.0)


# ---- 1. the helper against what exists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w7_gen", "resumed", "underfilled"])
def test_without_checks_the_helper_is_the_unchecked_beams(name):
    got, want = bcref.run(name, dict(checks=0)), bref.reference(name)
    for q in ("n_live", "path", "score", "penalty", "state"):
        assert np.ascontiguousarray(got[q]).tobytes() == np.ascontiguousarray(want[q]).tobytes(), (name, q)
    assert got["base_penalty"].tobytes() == want["penalty"].tobytes() and not got["hit"].any() and not got["sums"]
    for key in bref.PLAN_KEYS:
        assert got["plan"][key].tobytes() == want["plan"][key].tobytes(), (name, key)
    for b, root in enumerate(got["log"]):
        for s, sg in enumerate(root):
            assert sg["survivors"] == want["log"][b][s]["survivors"] == sg["unchecked"]


def test_a_checked_beam_that_prunes_nothing_holds_the_brute_force_minimum():
    """W >= M ** S, no reject bit: every path survives, in score order.  All M ** S paths enumerated from resume_batch, each scored
    on its WHOLE path at once — the summaries of the S * k cycles from the root's feet, folded once onto the accumulated penalty:
    that the beam's per-segment carry gives the same is the point."""
    name = "underfilled"
    c = bcref.base_case(name)
    env, checks, feet = bcref.environment(c), bcref.checks_of(name, reject=0), bcref.start_feet(name)
    M, S, k, W = c["M"], c["S"], c["k"], 9
    assert W >= M ** S
    got = bcref.beam(env, c["oroots"], c["options"], S, k, W, c["weights"], checks, feet)
    assert got["n_live"].tolist() == [M ** S] * c["B"]
    for b in range(c["B"]):
        brute = {}
        for path in itertools.product(range(M), repeat=S):
            state = rref.states_from_poses(c["oparams"], c["oroots"][b:b + 1], c["options"][path[0]:path[0] + 1])
            penalty, parts = 0.0, []
            for m in path:
                plan, states = rref.resume_batch(env["omap"], c["oparams"], c["oroots"][b:b + 1], state, k, c["options"][m:m + 1])
                penalty = penalty + bref.segment_penalty({key: v[0] for key, v in plan.items()}, k, c["weights"])
                state = states[-1]
                parts.append(plan)
            nominal, ok = np.concatenate([q["nominal"] for q in parts], axis=1), np.concatenate([q["cycle_ok"] for q in parts], axis=1)
            v = cref.fold(np.array([penalty]), np.zeros(1), bcref.path_summaries(env, nominal, ok, feet[b:b + 1], checks), checks)["score"][0]
            brute[path] = (bref.candidate_score(float(v), state[0], c["weights"])[0], float(v), penalty)
        assert got["score"][b, 0] == min(sc for sc, _, _ in brute.values())
        assert (np.diff(got["score"][b]) >= 0).all()
        for w in range(M ** S):
            assert brute[tuple(got["path"][b, w].tolist())] == (got["score"][b, w], got["penalty"][b, w], got["base_penalty"][b, w]), (b, w)
    plain = bref.beam(env["omap"], c["oparams"], c["oroots"], c["options"], S, k, W, c["weights"])
    assert got["path"].tolist() != plain["path"].tolist()   # the check terms reorder the same M ** S paths


@pytest.mark.parametrize("name", bcref.CASES)
def test_final_slots_hold_the_summaries_hit_and_feet_of_their_full_products(name):
    """The contract, on the helper: for every final slot, the three summaries are rank_checked_reference.summaries on the slot's
    concatenated products from the root's start feet, `hit` is the fold's, `feet` the last committed cycle's records."""
    c, ref = bcref.base_case(name), bcref.reference(name)
    env, checks, feet = bcref.environment(c), bcref.checks_of(name), bcref.start_feet(name)
    n = int(ref["n_live"][0])
    for b in range(c["B"]):
        nominal, ok = ref["plan"]["nominal"][b], ref["plan"]["cycle_ok"][b]
        assert nominal.shape[:2] == (n, c["S"] * c["k"])
        want = bcref.path_summaries(env, nominal, ok, np.broadcast_to(feet[b], (n, 4, 3)), checks)
        for q in ("swing", "trunk", "margin"):
            assert ref["sums"][q][b].tobytes() == want[q].tobytes(), (name, b, q)
        fold = cref.fold(ref["base_penalty"][b], np.zeros(n), want, checks)
        assert np.array_equal(fold["hit"], ref["hit"][b])
        finite = np.isfinite(ref["score"][b])
        assert np.array_equal(fold["score"][finite], ref["penalty"][b][finite])
        for w in range(n):
            assert np.array_equal(ref["feet"][b, w], bcref.carried_feet(nominal[w], ok[w], feet[b]), equal_nan=True)


# ---- 2. the GPU tests' inputs ------------------------------------------------------------------------------------------------------------
# which case carries which condition (found by running the helper; a case's row, roots and options decide what it can show).  Every
# condition has at least one carrier — asserted below — and every carrier is asserted to show it.
ALWAYS = {"checked_survivors_differ_from_the_unchecked", "an_exact_tie_at_a_survivor"}
SHOWS = {
    "w7_gen": {"class_0_and_class_1_in_one_segment", "only_class_1_and_still_full_in_score_order", "a_global_first_cycle"},
    "w7_gen_k5": {"class_0_and_class_1_in_one_segment"},
    "w16_seq": {"class_0_and_class_1_in_one_segment", "only_class_1_and_still_full_in_score_order", "every_hit_bit_set_and_clear",
                "a_global_first_cycle"},
    "w48_direct": {"class_0_and_class_1_in_one_segment"},
    "underfilled": {"class_0_and_class_1_in_one_segment", "only_class_1_and_still_full_in_score_order", "every_hit_bit_set_and_clear",
                    "a_global_first_cycle"},
    "resumed": {"class_0_and_class_1_in_one_segment", "a_candidate_without_commits_inherits_its_parents_feet"},
    "largest_sort": {"class_0_and_class_1_in_one_segment"},
    "nan_option": {"class_0_and_class_1_in_one_segment", "every_hit_bit_set_and_clear", "a_global_first_cycle"},
    "stance_start": {"only_class_1_and_still_full_in_score_order", "every_hit_bit_set_and_clear", "a_global_first_cycle"},
    "w48_raised": {"class_0_and_class_1_in_one_segment", "a_negative_max_lift"},
}
CONDITIONS = ALWAYS | {"class_0_and_class_1_in_one_segment", "only_class_1_and_still_full_in_score_order", "every_hit_bit_set_and_clear",
                       "a_candidate_without_commits_inherits_its_parents_feet", "a_negative_max_lift", "a_global_first_cycle"}


def test_every_condition_has_a_carrier():
    assert set(SHOWS) == set(bcref.CASES)
    assert ALWAYS.union(*SHOWS.values()) == CONDITIONS


@pytest.mark.parametrize("name", bcref.CASES)
def test_gpu_inputs_exercise_what_the_checked_beam_adds(name):
    """Every case tests/test_gpu_beam_checked.py runs: in some segment the checked survivors are not what the unchecked order keeps
    from the same candidates, an exact score tie involves a survivor, and the case shows every condition SHOWS names for it: class 0
    beside class 1 in one segment; a root with only class 1 candidates that still fills its slots in score order; every hit bit set
    in one final slot and clear in another; a candidate that commits nothing, keeps its parent's feet and has a child whose first
    swing starts there; a path with a negative max_lift; a final first_*_cycle >= k; an exact tie at a survivor."""
    c, ref = bcref.base_case(name), bcref.reference(name)
    cond = bcref.conditions(ref, c["k"])
    assert set(cond) == CONDITIONS
    missing = {what for what in ALWAYS | SHOWS[name] if not cond[what]}
    assert not missing, (name, missing)
    n = [min(c["W"], c["M"] ** (s + 1)) for s in range(c["S"])]
    assert [len(sg["survivors"]) for sg in ref["log"][0]] == n and (ref["n_live"] == n[-1]).all()
    for root in ref["log"]:   # counts only grow along a path: the children of a rejected survivor are rejected
        for s in range(1, c["S"]):
            prev, sg = root[s - 1], root[s]
            for w, pc in enumerate(prev["survivors"]):
                if prev["classes"][pc] == 1:
                    assert all(cl >= 1 for cl in sg["classes"][w * c["M"]:(w + 1) * c["M"]])
    if name == "nan_option":   # the NaN start's four children: class 2, by index, behind every finite candidate
        assert np.isfinite(ref["score"][:, :12]).all() and np.isnan(ref["score"][:, 12:]).all()
        assert ref["path"][:, 12:].tolist() == [[[1, m] for m in range(4)]] * c["B"]
        assert all(root[-1]["classes"][12:] == [2] * 4 for root in ref["log"])
    else:
        assert np.isfinite(ref["score"]).all() and np.isfinite(ref["penalty"]).all()
    if name == "w48_raised":
        sw = ref["sums"]["swing"]
        assert ((sw["max_lift"] < 0) & (sw["n_segments"] > 0)).any()   # ... and it reaches a final slot


def test_the_limits_come_from_the_data_and_split_it():
    """max_lift and min_clearance are medians over the unchecked beam's candidates: about half of the candidates with a segment lie on
    either side"""
    for name in ("w7_gen", "w16_seq", "w48_direct"):
        lim = bcref.limits(name)
        segs = [sg["segment"] for root in bcref.free_reference(name)["log"] for sg in root]
        lift = np.concatenate([sg["swing"]["max_lift"][sg["swing"]["n_segments"] > 0] for sg in segs])
        assert 0 < np.count_nonzero(lift > lim["swing"]["max_lift"]) < lift.size, name
        assert lim["trunk"]["ride_height"] == 0.25 and lim["margin"] == cref.MARGIN_LIMIT
