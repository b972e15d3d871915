"""The checked ranking (include/fpe.h, "checked ranking") without a GPU: the binding against the library and the header compiled as
plain C, the defaults, tests/rank_checked_reference.py by hand on synthetic summaries, and the main case of the GPU tests kept from
being hollow — on the oracle and the references alone."""
import ctypes as C
import functools
import re

import numpy as np

from oracle import fpo
from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import make_check_params, make_margin_params, make_swing_limits, make_trunk_limits
from tests import abi_c
from tests import margin_reference
from tests import rank_checked_reference as ref
from tests import rank_reference
from tests import util
from tests.conftest import yaml_params

SYMBOLS = ("fpe_check_params_defaults", "fpe_check_plan_device", "fpe_plan_rank_checked_device", "fpe_plan_rank_checked")


def test_every_symbol_is_in_the_binding_and_in_the_library():
    with open(abi_c.ROOT + "/include/fpe.h") as f:
        declared = set(re.findall(r"^int (fpe_check_\w+|fpe_plan_rank_checked\w*)\(", f.read(), re.M))
    assert declared == set(SYMBOLS)
    lib = _capi.lib()
    for name in SYMBOLS:
        assert name in _capi.PROTOTYPES and name in _capi.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    assert "fpe_check_params" in _capi.STRUCTS and "fpe_check_out" in _capi.STRUCTS
    assert _capi.ABI_VERSION == 5 and lib.fpe_abi_version() == 5
    assert (_capi.CHECK_SWING, _capi.CHECK_TRUNK, _capi.CHECK_MARGIN, _capi.CHECK_UNKNOWN) == (1, 2, 4, 8)


def test_defaults_are_the_documented_values():
    cp = _capi.CheckParams()
    C.memset(C.byref(cp), 0x5B, C.sizeof(cp))
    assert _capi.lib().fpe_check_params_defaults(C.byref(cp)) == _capi.FPE_OK
    assert (cp.checks, cp.reject) == (7, 0)
    assert (cp.w_swing_over, cp.w_lift, cp.w_trunk_bad, cp.w_margin_under, cp.w_unknown) == (10.0, 0.0, 10.0, 1.0, 1.0)
    assert bytes(C.c_double(cp.reserved)) == bytes(8)
    sl, tl, mp = _capi.SwingLimits(), _capi.TrunkLimits(), _capi.MarginParams()
    lib = _capi.lib()
    assert (lib.fpe_swing_limits_defaults(C.byref(sl)), lib.fpe_trunk_limits_defaults(C.byref(tl)), lib.fpe_margin_params_defaults(C.byref(mp))) == (0, 0, 0)
    assert bytes(cp.swing) == bytes(sl) and bytes(cp.trunk) == bytes(tl) and bytes(cp.margin) == bytes(mp)
    assert lib.fpe_check_params_defaults(None) == _capi.FPE_E_INVALID_ARG
    # the Python constructor agrees with the library byte for byte, and the reference's defaults are the same values
    assert bytes(make_check_params()) == bytes(cp) == bytes(_capi.check_params_defaults())
    d = ref.DEFAULT_CHECKS
    assert (d["checks"], d["reject"], d["w_swing_over"], d["w_lift"], d["w_trunk_bad"], d["w_margin_under"], d["w_unknown"]) == (
        7, 0, 10.0, 0.0, 10.0, 1.0, 1.0)
    named = make_check_params(checks=("swing", "margin"), reject=("margin", "unknown"), swing=dict(max_lift=0.1),
                              trunk=make_trunk_limits(ride_height=0.2), margin=make_margin_params(13, 4, 0.01))
    assert (named.checks, named.reject, named.swing.max_lift, named.trunk.ride_height, named.margin.reach_cells) == (5, 12, 0.1, 0.2, 4)
    assert bytes(named.swing) == bytes(make_swing_limits(max_lift=0.1))


def test_the_header_is_plain_c_with_the_documented_layout(tmp_path):
    body = r'''
  printf("abi %d\n", FPE_ABI_VERSION);
  printf("params %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fpe_check_params), offsetof(fpe_check_params, checks),
         offsetof(fpe_check_params, reject), offsetof(fpe_check_params, w_swing_over), offsetof(fpe_check_params, w_lift),
         offsetof(fpe_check_params, w_trunk_bad), offsetof(fpe_check_params, w_margin_under), offsetof(fpe_check_params, w_unknown),
         offsetof(fpe_check_params, reserved), offsetof(fpe_check_params, swing), offsetof(fpe_check_params, trunk),
         offsetof(fpe_check_params, margin));
  printf("out %zu %zu %zu %zu %zu %zu\n", sizeof(fpe_check_out), offsetof(fpe_check_out, swing), offsetof(fpe_check_out, trunk),
         offsetof(fpe_check_out, margin), offsetof(fpe_check_out, base_score), offsetof(fpe_check_out, hit));
  printf("consts %u %u %u %u\n", FPE_CHECK_SWING, FPE_CHECK_TRUNK, FPE_CHECK_MARGIN, FPE_CHECK_UNKNOWN);
'''
    decls = r'''
  { fpe_check_params p; fpe_check_out o = {0, 0, 0, 0, 0}; fpe_rank_out r; fpe_plan_out po; const double* feet = 0;
    const fpe_pose* poses = 0; const fpe_stride* strides = 0; const fpe_rank_params* rank = 0;
    int (*defaults)(fpe_check_params*) = fpe_check_params_defaults;
    int (*stage)(fpe_handle, const fpe_params*, const fpe_check_params*, const fpe_plan_out*, const double*, int32_t, int32_t,
                 const fpe_check_out*, void*) = fpe_check_plan_device;
    int (*device)(fpe_handle, const fpe_params*, const fpe_rank_params*, const fpe_check_params*, const fpe_pose*, const fpe_stride*,
                  int32_t, int32_t, int32_t, const fpe_plan_out*, const fpe_rank_out*, const fpe_check_out*, void*) =
        fpe_plan_rank_checked_device;
    int (*host)(fpe_handle, const fpe_params*, const fpe_rank_params*, const fpe_check_params*, const fpe_pose*, const fpe_stride*,
                int32_t, int32_t, int32_t, const fpe_rank_out*, const fpe_check_out*) = fpe_plan_rank_checked;
    (void)defaults(&p); (void)stage(0, 0, &p, &po, feet, 1, 1, &o, 0);
    (void)device(0, 0, rank, &p, poses, strides, 1, 1, 1, &po, &r, &o, 0); (void)host(0, 0, rank, &p, poses, strides, 1, 1, 1, &r, &o); }
'''
    out = abi_c.compile_and_run(tmp_path, body, decls)
    print(out)
    assert out.splitlines() == ["abi 5", "params 160 0 4 8 16 24 32 40 48 56 88 136", "out 40 0 8 16 24 32", "consts 1 2 4 8"]
    assert (C.sizeof(_capi.CheckParams), C.sizeof(_capi.CheckOut)) == (160, 40)
    assert [getattr(_capi.CheckParams, k).offset for k, _ in _capi.CheckParams._fields_] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 88, 136]


# ---- the reference by hand, on six synthetic summaries -------------------------------------------------------------------------------
def synthetic():
    """Six poses, all of base score 3.0 unless stated, nine cycles each"""
    S = np.zeros(6, _capi.SWING_SUMMARY_DTYPE)
    T = np.zeros(6, _capi.TRUNK_SUMMARY_DTYPE)
    M = np.zeros(6, _capi.MARGIN_SUMMARY_DTYPE)
    S["n_over"] = [0, 2, 0, 0, 0, 0]
    S["max_lift"] = [0.0, 0.5, 0.0, 0.0, 0.0, 0.25]
    S["n_unknown"] = [0, 0, 0, 0, 1, 0]
    T["n_bad"] = [0, 0, 1, 0, 0, 0]
    T["n_unknown"] = [0, 0, 0, 0, 2, 0]
    T["min_clearance"] = np.inf
    M["n_under"] = [0, 0, 0, 3, 0, 0]
    M["n_off_map"] = [0, 0, 0, 0, 4, 0]
    base = np.full(6, 3.0)
    succeed = np.full(6, 9)
    return base, succeed, dict(swing=S, trunk=T, margin=M)


def test_reference_chain_hits_and_the_tie_falling_to_the_index():
    base, succeed, sums = synthetic()
    out = ref.fold(base, succeed, sums)
    # 3 | 3 + 10 * 2 | 3 + 10 | 3 + 3 | 3 + 7 | 3
    assert out["score"].tolist() == [3.0, 23.0, 13.0, 6.0, 10.0, 3.0]
    assert out["hit"].tolist() == [0, ref.SWING, ref.TRUNK, ref.MARGIN, ref.UNKNOWN, 0] and out["unknown"].tolist() == [0, 0, 0, 0, 7, 0]
    assert out["order"].tolist() == [0, 5, 3, 4, 2, 1] and out["cls"].tolist() == [0] * 6 and out["n_class0"] == 6  # 0 and 5 tie
    lifted = ref.fold(base, succeed, sums, dict(w_lift=4.0))
    assert lifted["score"].tolist() == [3.0, 25.0, 13.0, 6.0, 10.0, 4.0] and lifted["order"].tolist() == [0, 5, 3, 4, 2, 1]
    assert lifted["hit"].tolist() == out["hit"].tolist()


def test_reference_negative_zero_weights_give_positive_zero():
    base, succeed, sums = synthetic()
    zero = dict(w_swing_over=-0.0, w_lift=-0.0, w_trunk_bad=-0.0, w_margin_under=-0.0, w_unknown=-0.0)
    out = ref.fold(np.full(6, -0.0), succeed, sums, zero)
    assert np.all(out["score"] == 0.0) and not np.signbit(out["score"]).any()
    assert out["order"].tolist() == [0, 1, 2, 3, 4, 5]


def test_reference_each_reject_bit_alone_moves_its_pose_to_class_1():
    base, succeed, sums = synthetic()
    for bit, pose in ((ref.SWING, 1), (ref.TRUNK, 2), (ref.MARGIN, 3), (ref.UNKNOWN, 4)):
        out = ref.fold(base, succeed, sums, dict(reject=bit))
        assert out["cls"].tolist() == [1 if b == pose else 0 for b in range(6)], bit
        assert out["order"].tolist()[-1] == pose and out["n_class0"] == 5
        assert out["score"].tolist() == [3.0, 23.0, 13.0, 6.0, 10.0, 3.0]       # the score does not depend on `reject`
    out = ref.fold(base, succeed, sums, dict(reject=15))
    assert out["cls"].tolist() == [0, 1, 1, 1, 1, 0] and out["order"].tolist() == [0, 5, 3, 4, 2, 1] and out["n_class0"] == 2
    short = succeed.copy()
    short[0] = 2
    out = ref.fold(base, short, sums, dict(reject=ref.MARGIN), min_cycles=3)  # the ranking's own class-1 rule is OR-ed
    assert out["cls"].tolist() == [1, 0, 0, 1, 0, 0] and out["order"].tolist() == [5, 4, 2, 1, 0, 3]


def test_reference_an_overflowing_unknown_term_is_class_2():
    base, succeed, sums = synthetic()
    out = ref.fold(base, succeed, sums, dict(w_unknown=1e308, reject=15))
    assert np.isinf(out["score"][4]) and out["cls"].tolist() == [0, 1, 1, 1, 2, 0]
    assert out["order"].tolist() == [0, 5, 3, 2, 1, 4] and out["n_class0"] == 2


def test_reference_no_check_is_the_plain_ranking_and_a_disabled_checks_summary_is_ignored():
    s = np.zeros(6, _capi.POSE_SUMMARY_DTYPE)
    s["committed"] = [9, 9, 8, 9, 9, 2]
    s["gait_cycles_succeed"] = [9, 9, 9, 9, 9, 2]
    s["n_source"][:, 1] = [3, 1, 0, 1, 0, 0]
    _, _, sums = synthetic()
    for rank in (None, dict(min_cycles=3), dict(w_deviation=1e308)):
        score, cls, order, n0 = rank_reference.score_and_order(s, rank, 9)
        out = ref.checked(s, rank, 9, sums, dict(checks=0))
        assert out["score"].tobytes() == score.tobytes() == out["base_score"].tobytes()
        assert (out["cls"].tolist(), out["order"].tolist(), out["n_class0"]) == (cls.tolist(), order.tolist(), n0)
        assert not out["hit"].any()
    # garbage in the summaries of disabled checks changes nothing
    base, succeed, sums = synthetic()
    want = ref.fold(base, succeed, sums, dict(checks=ref.TRUNK, reject=ref.TRUNK | ref.UNKNOWN))
    assert want["score"].tolist() == [3.0, 3.0, 13.0, 3.0, 5.0, 3.0] and want["hit"].tolist() == [0, 0, 2, 0, 8, 0]
    garbage = dict(sums)
    garbage["swing"] = np.frombuffer(b"\x5b" * sums["swing"].nbytes, _capi.SWING_SUMMARY_DTYPE)
    garbage["margin"] = np.frombuffer(b"\xff" * sums["margin"].nbytes, _capi.MARGIN_SUMMARY_DTYPE)
    got = ref.fold(base, succeed, garbage, dict(checks=ref.TRUNK, reject=ref.TRUNK | ref.UNKNOWN))
    assert all(np.array_equal(got[k], want[k]) for k in ("score", "hit", "unknown", "cls", "order"))
    del garbage["swing"], garbage["margin"]
    assert np.array_equal(ref.fold(base, succeed, garbage, dict(checks=ref.TRUNK))["score"], want["score"])


# ---- the main case of the GPU tests, on the oracle alone -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_case():
    trav, elev, res, poses, n = ref.real_inputs()
    omap = fpo.OracleMap(trav, elev, res)
    p, op = yaml_params(), util.to_oracle_poses(poses)
    plan = omap.plan(p, op, n, threads=4)
    summary = rank_reference.summary_from_oracle(omap, p, op, n, plan=plan)
    thr = margin_reference.thresholds(p)
    limits = ref.derived_limits(trav, elev, res, thr, plan["nominal"], plan["cycle_ok"], plan["stance"])
    sums = ref.summaries(trav, elev, res, (0.0, 0.0), thr, plan["nominal"], plan["cycle_ok"], plan["stance"], limits)
    return summary, sums, limits, n


def test_main_inputs_keep_the_checked_ranking_from_being_trivial():
    summary, sums, limits, n = main_case()
    B = summary.shape[0]
    assert B == 72
    out = ref.checked(summary, None, n, sums, dict(limits, reject=15))
    for bit in (ref.SWING, ref.TRUNK, ref.MARGIN, ref.UNKNOWN):  # every hit bit set for at least 8 poses and clear for at least 8
        hits = int(np.count_nonzero(out["hit"] & bit))
        print("bit", bit, "hit / miss", hits, B - hits)
        assert 8 <= hits <= B - 8, (bit, hits)
    print("class 0 with four reject bits:", out["n_class0"])
    assert 1 <= out["n_class0"] <= 15
    free = ref.checked(summary, None, n, sums, limits)   # the default weights, no reject bit
    plain = rank_reference.score_and_order(summary, None, n)
    assert free["base_score"].tobytes() == plain[0].tobytes()
    top, top_plain = free["order"][:16].tolist(), plain[2][:16].tolist()
    assert top != top_plain and len(set(free["score"][top].tolist())) == 16
