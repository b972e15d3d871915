"""The engine, through the C ABI, against the REFERENCE's own planner: tests/golden/ref/*.npz only (what the reference's
FootholdPlanner.cpp, compiled verbatim against oracle/ref_shim/, computed — tests/golden/make_ref_golden.py).  Neither
the reference tree nor the oracle is consulted.  Bar: integers, flags, x and y exact, |dz| <= util.Z_TOL.

What a fixture can say about a plan is what the reference publishes: the footholds of the COMMITTED cycles of an
accepted call (all three tracks), the stance, the feet-centre paths up to the last commit, every optimize() call, the
return value and the failing cycle."""
import os

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_poses
from tests import refcase, util

pytestmark = pytest.mark.gpu

NAMES = refcase.fixture_names()
SERVICE = [n for n in NAMES if n.startswith("svc_")]
LEGS = [n for n in NAMES if n.startswith("legs_")]

# describe_plan() under automatic dispatch, for EVERY service fixture, from the rules of the plan matrix
# (tests/test_gpu_plan_matrix.py, tests/tie_fixtures.py; csrc/fpe_bits.hpp::bits_supported, bits_shape):
#   * a bit-window kernel applies when the foot disc's offset table can be proven (no lattice point on its circle), the disc has at
#     most 16 cells and its bounding box (2 ceil(rf / res) + 2)^2 fits the per-leg scratch: every fixture here (foot radii of 0.4 to
#     2 cells) except the 3.7-cell foot of svc_fine_5mm (45 cells, box 100) and the exactly-one-cell foot of svc_tie_r5_k4_rf1;
#   * a window of up to 15 columns takes the 8-lane kernel <2, *> (k = 4 and 6 cells at 2^-5 m: 2 (k + 1) + 1; the yaml 0.1 m at
#     2 cm: 13), more than 32 the one-wavefront kernel (0.15 m at 1 cm: 16 cells each way); a foot radius inside the 3x3-only band
#     [0.9, 1] cell is the MID variant (15/16 cell; the yaml 0.02 m at 2 cm, which f32 holds a hair below one cell).
KERNELS = {
    "svc_tie_r5_k4_half": "plan_bits_kernel<2, false>",
    "svc_tie_r5_k6_mid": "plan_bits_kernel<2, true>",
    "svc_tie_r5_k4_rf1": "plan_chained_kernel",
    "svc_trot_2cm": "plan_bits_kernel<2, true>",
    "svc_harsh_2cm": "plan_bits_kernel<2, true>",
    "svc_trot_1cm_r015": "plan_bits_seq_kernel<1, 2>",
}
NO_BITS = ("svc_fine_5mm", "svc_tie_r5_k4_rf1")


def expected_kernel(name):
    """(prefix describe_plan() must start with, whether it must be a bit-window kernel)."""
    for k, v in KERNELS.items():
        if name == k or name.startswith(k + "_"):
            return v, v.startswith("plan_bits")
    return ("plan_", False) if name in NO_BITS else ("plan_bits", True)


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def fixtures():
    return {n: refcase.load_fixture(os.path.join(refcase.GOLDEN_DIR, n + ".npz")) for n in NAMES}


def _load(planner, fx, variant=None):
    planner.set_tuning(plan_group=0, literal_discs=0, no_bits=0, no_mid_variant=0)
    planner.params = np.array(fx["params"], dtype=_capi.PARAMS_DTYPE).reshape(1)
    planner.opt_params = _capi.opt_params_yaml()
    if variant is not None:
        assert _capi.OPT_PARAMS_DTYPE.itemsize == fx[variant + "/opt_params"].dtype.itemsize
        planner.opt_params = np.ascontiguousarray(fx[variant + "/opt_params"]).view(_capi.OPT_PARAMS_DTYPE).copy()
    planner.gridmapCallback(fx["trav"], fx["elev"], float(fx["res"]), tuple(fx["position"]))


def _assert_xyz(got_x, got_y, got_z, want, what):
    want = np.asarray(want, np.float64).reshape(-1, 3)
    assert not util._neq(np.asarray(got_x, np.float64).ravel(), want[:, 0]).any(), f"{what}: x differs"
    assert not util._neq(np.asarray(got_y, np.float64).ravel(), want[:, 1]).any(), f"{what}: y differs"
    dz = np.abs(np.asarray(got_z, np.float64).ravel() - want[:, 2])
    assert np.all(dz <= util.Z_TOL), f"{what}: max |dz| = {dz.max()}"


def _check_plan(eng, ref, N, what):
    """The chained plan against what the reference published for the same start poses."""
    for b in range(ref["ret"].size):
        w = f"{what} pose {b}"
        ok = eng["cycle_ok"][b].astype(bool)
        if not ref["ret"][b]:
            # refused in cycle `gate`: the nominal path was last published by the last commit before it
            gate = int(ref["fail_cycle"][b])
            com = np.nonzero(ok[:gate])[0]
            assert int(ref["nominal_path_n"][b]) == (int(com[-1]) + 1 if com.size else -1), w
            continue
        nf = int(ref["nominal_head"][b, 4])
        ids = ref["nominal_id"][b, 4:nf]
        com = np.unique(ids[:, 1]) if nf > 4 else np.zeros(0, np.int64)
        assert np.array_equal(np.nonzero(ok)[0], com), f"{w}: cycle_ok {ok.astype(int)} vs committed cycles {com}"
        assert np.array_equal(eng["stance"][b], ref["nominal_xyz"][b, :4]), f"{w}: stance"
        n = eng["nominal"][b][ok]
        assert (n["valid"] == 1).all() and (n["source"] <= 1).all(), w
        assert np.array_equal(n["foot_id"].ravel(), ids[:, 0]) and np.array_equal(n["gait_cycle_id"].ravel(), ids[:, 1]), w
        _assert_xyz(n["x"], n["y"], n["z"], ref["nominal_xyz"][b, 4:nf], w + " nominal")
        c = eng["centroid"][b][ok]
        _assert_xyz(c["x"], c["y"], c["z"], ref["centroid_xyz"][b, 4:nf], w + " centroid")
        assert int(ref["centroid_head"][b, 4]) == nf


@pytest.mark.parametrize("mode", ["auto", "no_bits", "no_mid_variant"])
@pytest.mark.parametrize("name", SERVICE)
def test_plan(planner, fixtures, name, mode):
    fx = fixtures[name]
    v = str(fx["variants"][0])  # the nominal and centroid tracks do not depend on the optimiser's parameters
    _load(planner, fx)
    N = int(fx["n_cycles"])
    try:
        if mode != "auto":
            planner.set_tuning(**{mode: 1})
        eng = planner.plan(make_poses(fx["poses"]), N)
        d = planner.describe_plan()
        if mode == "auto":
            prefix, bits = expected_kernel(name)
            assert d.startswith(prefix) and d.startswith("plan_bits") == bits, (name, prefix, d)
        if mode == "no_bits":
            assert not d.startswith("plan_bits"), (name, d)
        if mode == "no_mid_variant":
            assert not d.startswith("plan_bits_kernel") or ", true>" not in d.split("(")[0], (name, d)
        _check_plan(eng, refcase.variant(fx, v), N, f"{name} [{mode}: {d.split('(')[0].strip()}]")
    finally:
        planner.set_tuning(no_bits=0, no_mid_variant=0)


@pytest.mark.parametrize("name", LEGS)
def test_open_loop_legs(planner, fixtures, name):
    """search_legs (checkFoothold, per-query radius and rectangle) and centroid_legs against the `legs` fixtures."""
    fx = fixtures[name]
    _load(planner, fx)
    q, r = fx["queries"], fx["result"]
    k0 = q["kind"] == 0
    eq = np.zeros(int(k0.sum()), _capi.QUERY_DTYPE)
    eq["cx"], eq["cy"], eq["search_radius"], eq["n_vertices"] = q["cx"][k0], q["cy"][k0], q["search_radius"][k0], 4
    eq["vx"][:, :4], eq["vy"][:, :4] = q["vx"][k0], q["vy"][k0]
    assert (q["foot_radius"][k0] == fx["params"]["footRadius"][0]).all()
    got = planner.checkFoothold(eq)
    assert np.array_equal(got["valid"], r[k0, 0].astype(np.uint8)), name
    assert np.array_equal(got["source"], r[k0, 1].astype(np.uint8)), name
    _assert_xyz(got["x"], got["y"], got["z"], r[k0][:, 2:5], name + " checkFoothold")
    assert len(set(got["source"].tolist())) == 3, "default, candidate and none each occur"
    k1 = q["kind"] == 1
    cq = np.zeros(int(k1.sum()), _capi.CENTROID_QUERY_DTYPE)
    cq["cx"], cq["cy"] = q["cx"][k1], q["cy"][k1]
    cen = planner.centroid_legs(cq)
    rc = r[k1]
    untouched = np.isnan(rc[:, 2])
    assert np.array_equal(cen["code"] >= 5, untouched), name
    t = ~untouched
    _assert_xyz(cen["x"][t], cen["y"][t], cen["z"][t], rc[t][:, 2:5], name + " centroid method")
    # the reference's outputs alone tell whole-region-valid (0) from a case (1-4), no case (5) and no submap (6)
    cls = refcase.reference_centroid_class(r)[k1]
    assert np.array_equal(np.where((cen["code"] >= 1) & (cen["code"] <= 4), 1, cen["code"]), cls), name


@pytest.mark.parametrize("name", SERVICE)
def test_plan_opt(planner, fixtures, name):
    """Every optimize() call of the reference: the problem (submap, indices, bounds, rows of the previous commit), the
    solution and its objective value (the reference's own nloptFunc evaluated it), the status, the failing cycle."""
    fx = fixtures[name]
    N = int(fx["n_cycles"])
    for v in fx["variants"]:
        v = str(v)
        _load(planner, fx, v)
        ref = refcase.variant(fx, v)
        poses = make_poses(fx["poses"])
        eng = planner.plan(poses, N, products=("cycle_ok",))
        o = planner.plan_opt(poses, N, eng["cycle_ok"])
        assert np.array_equal(o["gate_fail_cycle"], ref["fail_cycle"]), f"{name}/{v}: {o['gate_fail_cycle']} vs {ref['fail_cycle']}"
        for b in range(ref["ret"].size):
            n = int(ref["opt_n"][b])
            c, rr = o["cycles"][b][:n], ref["opt_rec"][b, :n]
            w = f"{name}/{v} pose {b}"
            for f, lo, hi in (("gait_top_left", 0, 2), ("gait_size", 2, 4), ("nominal_index", 4, 12), ("centroid_index", 12, 20),
                              ("x_lower", 20, 28), ("x_upper", 28, 36), ("x", 36, 44)):
                assert np.array_equal(c[f].reshape(n, hi - lo).astype(np.float64), rr[:, lo:hi]), f"{w}: {f}"
            assert not util._neq(c["minf"], rr[:, 44]).any(), f"{w}: minf {c['minf']} vs {rr[:, 44]}"
            assert np.array_equal(c["lf_current_row"], rr[:, 45]) and np.array_equal(c["rh_current_row"], rr[:, 46]), w
            assert np.array_equal(c["solver_status"].astype(np.float64), rr[:, 47]), f"{w}: status"
            assert (c["gate_failed"] == 0).all(), w
            if ref["ret"][b]:
                nf = int(ref["opt_head"][b, 4])
                f = o["footholds"][b][eng["cycle_ok"][b].astype(bool)]
                assert (f["committed"] == 1).all() and f.size == nf - 4, w
                _assert_xyz(f["x"], f["y"], f["z"], ref["opt_xyz"][b, 4:nf], w + " opt footholds")


@pytest.mark.parametrize("name", SERVICE)
def test_service_all_tracks(planner, fixtures, name):
    """globalFootholdPlan under service_opt_gate = 2: False exactly where the reference returned false, in the same
    cycle; otherwise the three messages and the feet-centre paths."""
    fx = fixtures[name]
    N = int(fx["n_cycles"])
    for v in fx["variants"]:
        v = str(v)
        _load(planner, fx, v)
        ref = refcase.variant(fx, v)
        for b, pos in enumerate(fx["poses"]):
            w = f"{name}/{v} pose {b}"
            res = util.service_enforced(planner, N, pos, all_tracks=True)
            gate = planner.last_service_gate()
            assert (res is False) == (ref["ret"][b] == 0), f"{w}: engine {res is not False}, reference {bool(ref['ret'][b])}"
            assert gate["fail_cycle"] == int(ref["fail_cycle"][b]), f"{w}: fail cycle {gate['fail_cycle']} vs {ref['fail_cycle'][b]}"
            if res is False:
                assert util.service_enforced(planner, N, pos) is False, w
                continue
            for t, m in (("nominal", res), ("centroid", res["centroid"]), ("opt", res["opt"])):
                pub, succ, gc, gcs, nf = (int(k) for k in ref[t + "_head"][b])
                assert pub == 1 and (m["success"], m["gait_cycles"], m["gait_cycles_succeed"]) == (bool(succ), gc, gcs), f"{w} {t}"
                f = m["footholds"]
                assert len(f) == nf, f"{w} {t}"
                assert np.array_equal(f["foot_id"], ref[t + "_id"][b, :nf, 0]) and np.array_equal(f["gait_cycle_id"], ref[t + "_id"][b, :nf, 1])
                _assert_xyz(f["x"], f["y"], f["z"], ref[t + "_xyz"][b, :nf], f"{w} {t} message")
            assert int(ref["response_n"][b]) == len(res["footholds"])
            # the paths as last published (on the last commit): a prefix of what the engine reports for all N cycles
            for key, path in (("nominal_path", res["report"]["path"]), ("centroid_path", res["centroid"]["report"]["path"])):
                n = int(ref[key + "_n"][b])
                if n > 0:
                    _assert_xyz(path[:n, 0], path[:n, 1], path[:n, 2], ref[key][b, :n], f"{w} {key}")
            assert np.array_equal(res["opt"]["cycles"]["x"].astype(np.float64), ref["opt_rec"][b, :N, 36:44]), w
