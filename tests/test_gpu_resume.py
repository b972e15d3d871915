"""Resumable plans on the GPU (fpe_plan_resume*, fpe_plan_state; include/fpe.h): every resume kernel family against the
oracle-derived reference of tests/resume_reference.py — never against an engine call of the whole horizon — on the rows and batches
of tests/stride_reference.py (an odd last 8-lane workgroup, a partly empty sixteen-pose workgroup), with splits on both sides of the
4-cycle y batch and of the 8-cycle flush.  That these inputs hold failed and committed cycles on both sides of every split is
checked on the oracle in tests/test_cpu_resume.py.  Bars: indices, flags, x / y, cycle_ok and every byte of the state exact,
|dz| <= 1e-6."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fpo
from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import PRODUCT_FIELDS, FootholdPlanner, make_plan_states, product_shapes
from tests import resume_reference as rref
from tests import util

pytestmark = pytest.mark.gpu

PRODUCTS = ("nominal", "centroid", "default", "cycle_ok", "selected", "selected_packed")  # what a continuation can return
FILL = 0xA5


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.set_max_leg_search_radius(0.0)
    p.close()


def use_case(planner, row_id, second_map=False):
    c = rref.case(row_id)
    planner.params = c["params"].copy()
    planner.set_max_leg_search_radius(float(c["row"].maxleg or 0.0))
    planner.gridmapCallback(c["trav2" if second_map else "trav"], c["elev2" if second_map else "elev"], c["row"].res)
    return c


def local_ids(eng, base):
    """The products of one segment with gait_cycle_id checked — state.cycle + g per pose — and rewritten to the call's own g, so
    that util.assert_products_equal's record checks apply to a segment as they do to a whole plan."""
    out = {k: v.copy() for k, v in eng.items()}
    for k in ("nominal", "selected"):
        if k in out:
            n = out[k].shape[1]
            want = (np.asarray(base, np.int64).reshape(-1, 1, 1) + np.arange(n).reshape(1, n, 1)) & 0xFF
            assert np.array_equal(out[k]["gait_cycle_id"], np.broadcast_to(want, out[k].shape)), f"{k}.gait_cycle_id is not state.cycle + g"
            out[k]["gait_cycle_id"] = np.arange(n, dtype=np.uint8)[:, None]
    return out


def concat(a, b):
    return {k: np.concatenate([a[k], b[k]], axis=1) for k in a}


def assert_states_equal(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    if got.tobytes() != ref.tobytes():
        for f in ("feet", "adjusted_y", "cycle", "reserved"):
            bad = np.nonzero(got[f].view(np.uint64 if got[f].dtype.itemsize == 8 else np.uint32) !=
                             ref[f].view(np.uint64 if ref[f].dtype.itemsize == 8 else np.uint32))
            assert bad[0].size == 0, f"{what}: state.{f}: {bad[0].size} mismatches, first at {tuple(b[0] for b in bad)}: " \
                                     f"{got[f][bad][0]!r} vs {ref[f][bad][0]!r}"
        raise AssertionError(f"{what}: state bytes differ")


# ---- 1. concatenation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", rref.SPLITS)
@pytest.mark.parametrize("row_id", rref.ROW_IDS)
def test_two_segments_are_the_oracles_chain(planner, row_id, k):
    """k cycles from the poses with the mixed strides, then N - k from the returned state with another stride array: both segments,
    their concatenation and both states are the reference's."""
    c = use_case(planner, row_id)
    d = planner.describe_plan(resume=True)
    assert d.startswith(rref.RESUME_KERNEL[row_id]), (row_id, d)
    ref = rref.reference(row_id, k)
    got1, st1 = planner.plan_resume(c["poses"], k, strides=c["mixed"], products=PRODUCTS)
    got2, st2 = planner.plan_resume(c["poses"], rref.N - k, states=st1, strides=c["mixed2"], products=PRODUCTS)
    try:
        util.assert_products_equal(local_ids(got1, 0), ref["first"], PRODUCTS)
        assert_states_equal(st1, ref["state_mid"], "first segment")
        util.assert_products_equal(local_ids(got2, k), ref["second"], PRODUCTS)
        assert_states_equal(st2, ref["state_end"], "second segment")
        util.assert_products_equal(concat(got1, got2), rref.concat(ref["first"], ref["second"]), PRODUCTS)  # ids 0 .. N - 1 as they are
    except AssertionError as e:
        raise AssertionError(f"{row_id}, B {c['B']}, k {k}, {d}: {e}") from None


@pytest.mark.parametrize("knob,kernel", [({"no_bits": 1}, "plan_chained_kernel<8, false> resume (direct"),
                                         ({"plan_group": 65}, "plan_sequential_kernel resume (direct")])
def test_direct_resume_kernels(planner, knob, kernel):
    c = use_case(planner, "w7_gen")
    ref = rref.reference("w7_gen", 5)
    with planner.tuning(**knob):
        assert planner.describe_plan(resume=True).startswith(kernel), planner.describe_plan(resume=True)
        got1, st1 = planner.plan_resume(c["poses"], 5, strides=c["mixed"], products=PRODUCTS)
        got2, st2 = planner.plan_resume(c["poses"], rref.N - 5, states=st1, strides=c["mixed2"], products=PRODUCTS)
    util.assert_products_equal(local_ids(got1, 0), ref["first"], PRODUCTS)
    util.assert_products_equal(local_ids(got2, 5), ref["second"], PRODUCTS)
    assert_states_equal(st1, ref["state_mid"], "first segment")
    assert_states_equal(st2, ref["state_end"], "second segment")


# ---- 2. replan on a new snapshot, in place, device form ---------------------------------------------------------------------------------
def device_resume(planner, poses, strides, states, n, products=PRODUCTS, in_place=True):
    """fpe_plan_resume_device on a stream of its own into sentinel-filled buffers: (products, state_out)."""
    B = poses.shape[0]
    shapes = product_shapes(B, n)
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    d_strides = torch.from_numpy(strides.view(np.uint8).copy()).cuda() if strides is not None else None
    d_state = torch.from_numpy(states.view(np.uint8).copy()).cuda()
    d_state_out = d_state if in_place else torch.full_like(d_state, FILL)
    out = {k: torch.full((int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize,), FILL, dtype=torch.uint8, device="cuda") for k in products}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        planner.plan_resume_device(d_poses.data_ptr(), B, n, {k: out[k].data_ptr() for k in products}, d_state_in_ptr=d_state.data_ptr(),
                                   d_state_out_ptr=d_state_out.data_ptr(), d_strides_ptr=d_strides.data_ptr() if d_strides is not None else 0,
                                   stream=stream.cuda_stream)
    stream.synchronize()
    return ({k: out[k].cpu().numpy().view(shapes[k][1]).reshape(shapes[k][0]) for k in products},
            d_state_out.cpu().numpy().view(_capi.PLAN_STATE_DTYPE).reshape(B))


@pytest.mark.parametrize("row_id", rref.ROW_IDS)
def test_replan_on_a_new_snapshot_in_place(planner, row_id):
    """4 cycles on the case's map, a second map of the same geometry uploaded, 5 more cycles from the state with state_out ==
    state_in: the helper on the second map, from the helper's own state of the first."""
    c = use_case(planner, row_id)
    ref = rref.reference(row_id, 4, second_map=True)
    got1, st1 = planner.plan_resume(c["poses"], 4, strides=c["mixed"], products=PRODUCTS)
    util.assert_products_equal(local_ids(got1, 0), ref["first"], PRODUCTS)
    assert_states_equal(st1, ref["state_mid"], row_id)
    use_case(planner, row_id, second_map=True)
    got2, st2 = device_resume(planner, c["poses"], c["mixed2"], st1, rref.N - 4)
    util.assert_products_equal(local_ids(got2, 4), ref["second"], PRODUCTS)
    assert_states_equal(st2, ref["state_end"], row_id)
    util.assert_products_equal(concat(got1, got2), rref.concat(ref["first"], ref["second"]), PRODUCTS)


# ---- 3. from feet -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", ["w7_mid", "w16_seq", "w48_direct"])
def test_from_feet(planner, row_id):
    """The four feet a robot stands on — here the cell centres of the first valid nominal foothold of each leg of a planned pose — as
    the state of all three tracks (fpe_plan_state_from_feet), 3 cycles with the parameters' stride, against the helper."""
    c = use_case(planner, row_id)
    nom = planner.plan(c["poses"], 8, products=("nominal",))["nominal"]
    omap = fpo.OracleMap(c["trav"], c["elev"], c["row"].res)
    keep, feet = [], []
    for b in range(c["B"]):
        if nom["valid"][b].any(axis=0).all():
            first = nom["valid"][b].argmax(axis=0)  # per leg: the first cycle with a valid foothold
            feet.append([omap.get_position(int(nom["row"][b, first[l], l]), int(nom["col"][b, first[l], l]))[1:] for l in range(4)])
            keep.append(b)
    assert len(keep) >= 3, len(keep)
    poses, oposes = c["poses"][keep], c["oposes"][keep]
    states = make_plan_states(None, feet=np.array(feet), adjusted_y=-0.01, cycle=6)
    got, st = planner.plan_resume(poses, 3, states=states, products=PRODUCTS)
    ref, ref_states = rref.resume_batch(omap, c["oparams"], oposes, states, 3)
    util.assert_products_equal(local_ids(got, 6), ref, PRODUCTS)
    assert_states_equal(st, ref_states[-1], row_id)
    assert (st["cycle"] == 9).all()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def raw_resume(planner, poses, states, n, products=PRODUCTS, strides=None):
    """fpe_plan_resume through the C ABI into sentinel-filled arrays: (status, outputs, state_out)."""
    B = poses.shape[0]
    shapes = product_shapes(B, max(int(n), 1))
    out = {k: np.full(int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize, FILL, np.uint8) for k in products}
    po = _capi.PlanOut()
    for k in out:
        setattr(po, PRODUCT_FIELDS[k], _capi.ptr(out[k]))
    state_out = np.full(B * _capi.PLAN_STATE_DTYPE.itemsize, FILL, np.uint8)
    rc = planner._lib.fpe_plan_resume(planner._h, _capi.ptr(planner.params), _capi.ptr(poses), _capi.ptr(strides), _capi.ptr(states), B, int(n),
                                      C.byref(po), _capi.ptr(state_out))
    return rc, out, state_out


def bad_states(base, what):
    s = base.copy()
    if what == "nan_foot":
        s["feet"][-1, 2, 1, 0] = np.nan
    elif what == "inf_foot_y":
        s["feet"][0, 0, 3, 1] = -np.inf
    elif what == "inf_adjusted_y":
        s["adjusted_y"][-1] = np.inf
    elif what == "reserved":
        s["reserved"][-1] = 1
    elif what == "negative_cycle":
        s["cycle"][1] = -1
    elif what == "cycle_past_255":
        s["cycle"][1] = 251  # + 5 cycles
    return s


@pytest.mark.parametrize("what", ["nan_foot", "inf_foot_y", "inf_adjusted_y", "reserved", "negative_cycle", "cycle_past_255", "n_cycles_0",
                                  "n_cycles_256", "stance", "pose_status"])
def test_host_form_refusals_write_nothing(planner, what):
    c = use_case(planner, "w7_gen")
    states = bad_states(rref.reference("w7_gen", 4)["state_mid"], what)
    n = {"n_cycles_0": 0, "n_cycles_256": 256}.get(what, 5)
    products = PRODUCTS + ((what,) if what in ("stance", "pose_status") else ())
    rc, out, state_out = raw_resume(planner, c["poses"], states, n, products)
    assert rc == _capi.FPE_E_INVALID_ARG, what
    assert all(np.all(v == FILL) for v in out.values()) and np.all(state_out == FILL)
    if what == "cycle_past_255":  # 250 + 5 is the last one taken
        states["cycle"][1] = 250
        rc, out, state_out = raw_resume(planner, c["poses"], states, n, products)
        assert rc == _capi.FPE_OK and state_out.view(_capi.PLAN_STATE_DTYPE)["cycle"][1] == 255


def test_forced_groups_without_a_resume_kernel_are_refused(planner):
    c = use_case(planner, "w7_gen")
    with planner.tuning(plan_group=16):
        rc, out, state_out = raw_resume(planner, c["poses"], rref.reference("w7_gen", 4)["state_mid"], 5)
        assert rc == _capi.FPE_E_UNSUPPORTED
        assert all(np.all(v == FILL) for v in out.values()) and np.all(state_out == FILL)
        rc, out, state_out = raw_resume(planner, c["poses"], None, 5)  # ... nor for a start that returns its state
        assert rc == _capi.FPE_E_UNSUPPORTED and np.all(state_out == FILL)
        planner.plan(c["poses"], 5)  # the plain call still runs there


# ---- 5. non-finite states in the device form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", rref.ROW_IDS)
def test_device_form_treats_a_half_finite_state_as_wholly_non_finite(planner, row_id):
    """One state with a NaN foot in the nominal track only (the last pose: the one an odd batch's padding slot replays), one with
    adjusted_y = inf, among finite neighbours: those two poses return, in every cycle, the records include/fpe.h lists for a
    non-finite step_length and NaN x in every track of state_out; everything else is the helper's, which implements the same rule."""
    c = use_case(planner, row_id)
    B, n = c["B"], 5
    states = rref.reference(row_id, 4)["state_mid"].copy()
    nan_pose, inf_pose = B - 1, 2
    states["feet"][nan_pose, 2, 1, 0] = np.nan
    states["adjusted_y"][inf_pose] = np.inf
    omap = fpo.OracleMap(c["trav"], c["elev"], c["row"].res)
    ref, ref_states = rref.resume_batch(omap, c["oparams"], c["oposes"], states, n, c["mixed2"])
    got, st = device_resume(planner, c["poses"], c["mixed2"], states, n, in_place=False)
    h = float(c["params"]["h"][0])
    for b in (nan_pose, inf_pose):
        nom, cen, dflt = got["nominal"][b], got["centroid"][b], got["default"][b]
        assert not nom["valid"].any() and (nom["source"] == 2).all() and (nom["row"] == -1).all() and (nom["col"] == -1).all()
        assert np.isnan(nom["x"]).all() and (~np.isfinite(nom["y"])).all() == (b == inf_pose)
        assert (cen["code"] == 6).all() and (cen["row"] == -1).all() and (cen["col"] == -1).all()
        assert (cen["x"] == 0).all() and (cen["y"] == 0).all() and (cen["z"] == 0).all()
        assert np.isnan(dflt[..., 0]).all() and (dflt[..., 2] == np.float32(0.0 + h)).all()
        assert not got["cycle_ok"][b].any()
        assert np.isnan(st["feet"][b, :, :, 0]).all() and st["cycle"][b] == 4 + n and st["reserved"][b] == 0
        assert st["feet"][b, :, :, 1].tobytes() == states["feet"][b, :, :, 1].tobytes()
    assert np.isinf(st["adjusted_y"][inf_pose]) and st["adjusted_y"][nan_pose] == ref_states[-1]["adjusted_y"][nan_pose]
    util.assert_products_equal(local_ids(got, 4), ref, PRODUCTS)  # (NaN == NaN there: the two poses, and every neighbour exactly)
    fine = np.ones(B, bool)
    fine[[nan_pose, inf_pose]] = False
    assert_states_equal(st[fine], ref_states[-1][fine], row_id)


# ---- 6. no state_in: fpe_plan_strides plus the state --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", rref.ROW_IDS)
def test_without_state_in_the_call_is_fpe_plan_strides_plus_the_state(planner, row_id):
    c = use_case(planner, row_id)
    n = max(rref.SPLITS)
    got, st = planner.plan_resume(c["poses"], n, strides=c["mixed"], products=util.ALL_PRODUCTS)
    plain = planner.plan(c["poses"], n, products=util.ALL_PRODUCTS, strides=c["mixed"])
    for k in util.ALL_PRODUCTS:
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(plain[k]).tobytes(), (row_id, k)
    assert_states_equal(st, rref.first_segment(row_id)[1][n - 1], row_id)
    # no strides either: every pose uses the stride of the parameters
    got0, st0 = planner.plan_resume(c["poses"], n, products=util.ALL_PRODUCTS)
    uniform = planner.plan(c["poses"], n, products=util.ALL_PRODUCTS, strides=c["uniform"])
    for k in util.ALL_PRODUCTS:
        assert np.ascontiguousarray(got0[k]).tobytes() == np.ascontiguousarray(uniform[k]).tobytes(), (row_id, k, "no strides")
    assert (st0["cycle"] == n).all()
    # ... and with neither state the call is fpe_plan_strides itself
    none, no_state = planner.plan_resume(c["poses"], n, strides=c["mixed"], products=util.ALL_PRODUCTS, want_state=False)
    assert no_state is None
    for k in util.ALL_PRODUCTS:
        assert np.ascontiguousarray(none[k]).tobytes() == np.ascontiguousarray(plain[k]).tobytes(), (row_id, k, "no states")
