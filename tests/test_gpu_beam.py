"""Beam search over stride options on the GPU (fpe_plan_beam*; include/fpe.h): both forms against the oracle-derived helper of
tests/beam_reference.py — path, n_live, penalty, score, state and every requested product byte for byte — on one row per plan-kernel
family, and against the engine's own fpe_plan_resume (the replay contract).  Every call writes into sentinel-filled buffers: dead
slots must keep the sentinel.  That the inputs hold pruning against the index order, failed cycles, exact ties, mixed paths and both
gaits is asserted on the helper alone in tests/test_cpu_beam.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import PRODUCT_FIELDS, FootholdPlanner, product_shapes
from tests import beam_reference as bref

pytestmark = pytest.mark.gpu

PRODUCTS = FootholdPlanner.BEAM_PRODUCTS
FILL = 0xA5
OWN = {"n_live": np.int32, "score": np.float64, "penalty": np.float64, "path": np.uint8, "state": _capi.PLAN_STATE_DTYPE}


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.set_max_leg_search_radius(0.0)
    p.close()


def use_case(planner, name):
    c = bref.case(name)
    planner.params = c["params"].copy()
    planner.set_max_leg_search_radius(float(c["row"].maxleg or 0.0))
    planner.gridmapCallback(c["trav"], c["elev"], c["row"].res)
    return c


def beam_params(c, **over):
    w = c["weights"]
    kw = dict(segments=c["S"], cycles_per_segment=c["k"], width=c["W"], w_fail=w[0], w_spiral=w[1], w_none=w[2], w_deviation=w[3], w_progress=w[4])
    kw.update(over)
    return _capi.beam_params_defaults(**kw)


def out_shapes(B, W, S, k, products):
    """name -> (shape, dtype) of every output of a beam call: its own five, then the products as [B, W, S * k, ...]."""
    shapes = {"n_live": ((B,), np.int32), "score": ((B, W), np.float64), "penalty": ((B, W), np.float64), "path": ((B, W, S), np.uint8),
              "state": ((B, W), _capi.PLAN_STATE_DTYPE)}
    ps = product_shapes(B * W, S * k)
    for q in products:
        shapes[q] = ((B, W) + ps[q][0][1:], ps[q][1])
    return shapes


def nbytes(shape, dtype):
    return int(np.prod(shape)) * np.dtype(dtype).itemsize


def beam_out(addr, products, skip=()):
    bo = _capi.BeamOut(*[addr[q] if q not in skip else None for q in OWN])
    for q in products:
        setattr(bo.products, PRODUCT_FIELDS[q], addr[q])
    return bo


def host_beam(planner, poses, options, bp, states=None, products=PRODUCTS, shape=None, skip=(), M=None, B=None):
    """fpe_plan_beam through the C ABI into sentinel-filled arrays: (status, outputs as typed [B, W, ...] views)."""
    S, k, W = shape or (bp.segments, bp.cycles_per_segment, bp.width)
    shapes = out_shapes(poses.shape[0], W, S, k, products)
    raw = {q: np.full(nbytes(*shapes[q]), FILL, np.uint8) for q in shapes}
    bo = beam_out({q: _capi.ptr(raw[q]) for q in raw}, products, skip)
    rc = planner._lib.fpe_plan_beam(planner._h, _capi.ptr(planner.params), C.byref(bp) if bp is not None else None, _capi.ptr(poses),
                                    _capi.ptr(states), poses.shape[0] if B is None else B, _capi.ptr(options), options.shape[0] if M is None else M,
                                    C.byref(bo))
    return rc, {q: raw[q].view(shapes[q][1]).reshape(shapes[q][0]) for q in raw}


def device_beam(planner, poses, options, bp, states=None, products=PRODUCTS):
    """fpe_plan_beam_device on a stream of its own into sentinel-filled device buffers: the outputs as typed [B, W, ...] views."""
    S, k, W = bp.segments, bp.cycles_per_segment, bp.width
    B = poses.shape[0]
    shapes = out_shapes(B, W, S, k, products)
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    d_options = torch.from_numpy(options.view(np.uint8).copy()).cuda()
    d_states = torch.from_numpy(states.view(np.uint8).copy()).cuda() if states is not None else None
    raw = {q: torch.full((nbytes(*shapes[q]),), FILL, dtype=torch.uint8, device="cuda") for q in shapes}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        planner.plan_beam_device(d_poses.data_ptr(), B, d_options.data_ptr(), options.shape[0], raw["path"].data_ptr(), beam=bp,
                                 d_state_in_ptr=d_states.data_ptr() if d_states is not None else 0, d_n_live_ptr=raw["n_live"].data_ptr(),
                                 d_score_ptr=raw["score"].data_ptr(), d_penalty_ptr=raw["penalty"].data_ptr(), d_state_ptr=raw["state"].data_ptr(),
                                 products={q: raw[q].data_ptr() for q in products}, stream=stream.cuda_stream)
    stream.synchronize()
    return {q: raw[q].cpu().numpy().view(shapes[q][1]).reshape(shapes[q][0]) for q in raw}


def run_form(planner, form, c, bp, products=PRODUCTS):
    if form == "device":
        return device_beam(planner, c["roots"], c["options"], bp, c["states"], products)
    rc, got = host_beam(planner, c["roots"], c["options"], bp, c["states"], products)
    assert rc == _capi.FPE_OK, planner._lib.fpe_last_error(planner._h)
    return got


def same_bits(a, b, nan_equal):
    """byte for byte; nan_equal: float fields that are NaN on both sides count as equal (a NaN's sign and payload are not specified)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.tobytes() == b.tobytes():
        return True
    if not nan_equal:
        return False
    if a.dtype.names:
        return all(same_bits(a[f], b[f], True) for f in a.dtype.names)
    if a.dtype.kind != "f":
        return False
    bits = "u8" if a.dtype.itemsize == 8 else "u4"
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))


def assert_beam_is(got, ref, products, what, nan_equal=False):
    """Every live slot of every output equals the helper's, byte for byte, and every dead slot still holds the sentinel."""
    n = int(ref["n_live"][0])
    assert got["n_live"].tolist() == ref["n_live"].tolist(), what
    want = {"score": ref["score"], "penalty": ref["penalty"], "path": ref["path"], "state": ref["state"]}
    want.update(bref.engine_products(ref, products))
    for q, w in want.items():
        live, dead = got[q][:, :n], got[q][:, n:]
        if not same_bits(live, w, nan_equal):
            bad = [(b, s) for b in range(w.shape[0]) for s in range(n) if not same_bits(live[b, s], w[b, s], nan_equal)]
            raise AssertionError(f"{what}: {q} differs in {len(bad)} live slots, first (root, slot) {bad[0]}: {live[bad[0]]!r} vs {w[bad[0]]!r}")
        assert np.all(np.ascontiguousarray(dead).view(np.uint8) == FILL), f"{what}: a dead slot of {q} was written"


# ---- 1. parity with the helper, both forms, one row per plan-kernel family --------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", ["w7_gen", "w7_gen_k5", "w16_seq", "w48_direct"])
def test_beam_is_the_helpers(planner, name, form):
    c = use_case(planner, name)
    d = planner.describe_plan(resume=True)
    assert d.startswith(bref.BEAM_KERNEL[c["row_id"]]), (name, d)
    got = run_form(planner, form, c, beam_params(c))
    assert_beam_is(got, bref.reference(name), PRODUCTS, f"{name}, {form} form, {d}")


# ---- 2. the replay contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w7_gen", "w7_gen_k5", "w16_seq", "w48_direct", "resumed"])
def test_replaying_every_slots_path_with_plan_resume_gives_its_products_and_state(planner, name):
    """All B * W live slots at once: S host plan_resume calls of k cycles with options[path[:, s]] and the state carried over."""
    c = use_case(planner, name)
    got = run_form(planner, "host", c, beam_params(c))
    B, W, S, k = c["B"], c["W"], c["S"], c["k"]
    assert (got["n_live"] == W).all()
    poses = np.repeat(c["roots"], W)
    states = None if c["states"] is None else np.repeat(c["states"], W)
    path = got["path"].reshape(B * W, S)
    parts = []
    for s in range(S):
        seg, states = planner.plan_resume(poses, k, states=states, strides=c["options"][path[:, s]], products=PRODUCTS)
        parts.append(seg)
    for q in PRODUCTS:
        replay = np.concatenate([seg[q] for seg in parts], axis=1)
        assert replay.tobytes() == np.ascontiguousarray(got[q]).tobytes(), (name, q)
    assert states.tobytes() == np.ascontiguousarray(got["state"]).tobytes(), name


# ---- 3. one option, one slot ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_one_option_one_slot_is_one_plan_resume(planner, form):
    c = use_case(planner, "degenerate")
    got = run_form(planner, form, c, beam_params(c))
    whole, state = planner.plan_resume(c["roots"], c["S"] * c["k"], strides=np.repeat(c["options"], c["B"]), products=PRODUCTS)
    assert got["n_live"].tolist() == [1] * c["B"] and not got["path"].any()
    for q in PRODUCTS:
        assert np.ascontiguousarray(got[q][:, 0]).tobytes() == whole[q].tobytes(), q
    assert np.ascontiguousarray(got["state"][:, 0]).tobytes() == state.tobytes()
    assert_beam_is(got, bref.reference("degenerate"), PRODUCTS, f"degenerate, {form} form")


# ---- 4. an underfilled beam ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", ["underfilled", "underfilled_s1"])
def test_underfilled_beam_leaves_dead_slots_alone(planner, name, form):
    """W = 8, M = 3.  S = 2: 3 entries, then 8 of 9.  S = 1: n_live = 3, and slots 3 .. 7 of every output keep the sentinel."""
    c = use_case(planner, name)
    got = run_form(planner, form, c, beam_params(c))
    ref = bref.reference(name)
    assert got["n_live"].tolist() == [8 if c["S"] == 2 else 3] * c["B"]
    assert_beam_is(got, ref, PRODUCTS, f"{name}, {form} form")


# ---- 5. the largest sort -------------------------------------------------------------------------------------------------------------
def test_largest_sort(planner):
    """B = 2, W = 64, M = 16, S = 3, k = 1: 16, 256 and 1024 keys per root."""
    c = use_case(planner, "largest_sort")
    got = run_form(planner, "device", c, beam_params(c), products=("nominal", "cycle_ok"))
    assert_beam_is(got, bref.reference("largest_sort"), ("nominal", "cycle_ok"), "largest sort")


# ---- 6. resumed roots ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_roots_resumed_from_an_earlier_plan(planner, form):
    c = use_case(planner, "resumed")
    _, states = planner.plan_resume(c["roots"], 3, products=("cycle_ok",))
    assert states.tobytes() == c["states"].tobytes()
    bp = beam_params(c)
    got = device_beam(planner, c["roots"], c["options"], bp, states) if form == "device" else host_beam(planner, c["roots"], c["options"], bp, states)[1]
    assert_beam_is(got, bref.reference("resumed"), PRODUCTS, f"resumed, {form} form")
    assert (got["nominal"]["gait_cycle_id"][:, :, 0] == 3).all() and (got["state"]["cycle"] == 3 + c["S"] * c["k"]).all()


# ---- 7. a non-finite option in the device form ---------------------------------------------------------------------------------------
def test_device_form_orders_non_finite_candidates_by_index_behind_the_finite_ones(planner):
    c = use_case(planner, "nan_option")
    got = device_beam(planner, c["roots"], c["options"], beam_params(c))
    assert np.isfinite(got["score"][:, :12]).all() and np.isnan(got["score"][:, 12:]).all()
    assert got["path"][:, 12:].tolist() == [[[1, m] for m in range(4)]] * c["B"]
    assert np.isnan(got["state"]["feet"][:, 12:, :, :, 0]).all()
    assert_beam_is(got, bref.reference("nan_option"), PRODUCTS, "NaN option", nan_equal=True)
    rc, out = host_beam(planner, c["roots"], c["options"], beam_params(c))  # the host form looks at the values
    assert rc == _capi.FPE_E_INVALID_ARG and all(np.all(v.view(np.uint8) == FILL) for v in out.values())


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def refusal_args(c, what):
    """(beam parameters, poses, options, states, products, keyword arguments of host_beam) of one refused call."""
    bp, poses, options, states, products, kw = beam_params(c), c["roots"].copy(), c["options"].copy(), None, PRODUCTS, {}
    if what in ("M_0", "M_17"):
        options = np.resize(options, 17)
        kw["M"] = 0 if what == "M_0" else 17
    elif what in ("W_0", "W_65"):
        bp.width = 0 if what == "W_0" else 65
        kw["shape"] = (c["S"], c["k"], 65)
    elif what == "S_0":
        bp.segments = 0
        kw["shape"] = (1, c["k"], c["W"])
    elif what == "k_0":
        bp.cycles_per_segment = 0
        kw["shape"] = (c["S"], 1, c["W"])
    elif what == "S_times_k_256":
        bp.segments, bp.cycles_per_segment = 16, 16
        kw["shape"] = (1, 1, c["W"])
    elif what == "B_0":
        kw["B"] = 0
    elif what == "too_many_chains":  # 3 * 64 * 16 fits; claim more roots than FPE_BEAM_MAX_CHAINS allows (refused before any is read)
        bp.width = 64
        options = np.resize(options, 16)
        kw["B"], kw["shape"] = (1 << 20) // (64 * 16) + 1, (c["S"], c["k"], 64)
    elif what == "reserved":
        bp.reserved = 1
    elif what == "nan_weight":
        bp.w_progress = float("nan")
    elif what == "inf_weight":
        bp.w_fail = float("inf")
    elif what == "no_path":
        kw["skip"] = ("path",)
    elif what in ("stance", "pose_status"):
        products = PRODUCTS + (what,)
    elif what == "nan_pose":
        poses["position"][1, 0] = np.nan
    elif what == "bad_gait":
        poses["gait"][2] = 2
    elif what == "inf_option":
        options["lateral_drift"][2] = np.inf
    elif what == "option_reserved":
        options["reserved"][0] = 1
    else:
        states = bref.case("resumed")["states"].copy()
        if what == "nan_state":
            states["feet"][1, 2, 0, 0] = np.nan
        elif what == "state_reserved":
            states["reserved"][0] = 1
        elif what == "negative_cycle":
            states["cycle"][2] = -1
        else:
            assert what == "cycle_past_255", what
            states["cycle"][2] = 255 - c["S"] * c["k"] + 1
    return bp, poses, options, states, products, kw


REFUSALS = ["M_0", "M_17", "W_0", "W_65", "S_0", "k_0", "S_times_k_256", "B_0", "too_many_chains", "reserved", "nan_weight", "inf_weight",
            "no_path", "stance", "pose_status", "nan_pose", "bad_gait", "inf_option", "option_reserved", "nan_state", "state_reserved",
            "negative_cycle", "cycle_past_255"]


@pytest.mark.parametrize("what", REFUSALS)
def test_host_form_refusals_write_nothing(planner, what):
    c = use_case(planner, "resumed")
    bp, poses, options, states, products, kw = refusal_args(c, what)
    rc, out = host_beam(planner, poses, options, bp, states, products, **kw)
    assert rc == _capi.FPE_E_INVALID_ARG, what
    assert all(np.all(v.view(np.uint8) == FILL) for v in out.values()), what
    if what == "cycle_past_255":  # one cycle earlier is the last state taken
        states["cycle"][2] -= 1
        rc, out = host_beam(planner, poses, options, bp, states, products)
        assert rc == _capi.FPE_OK and out["state"]["cycle"][2].tolist() == [255] * c["W"]


@pytest.mark.parametrize("what", ["M_17", "W_65", "S_times_k_256", "reserved", "nan_weight", "no_path", "stance"])
def test_device_form_refusals_queue_nothing(planner, what):
    c = use_case(planner, "resumed")
    bp, poses, options, _, products, kw = refusal_args(c, what)
    d_poses = torch.from_numpy(poses.view(np.uint8).copy()).cuda()
    d_options = torch.from_numpy(options.view(np.uint8).copy()).cuda()
    buf = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")  # every output pointer: nothing may be written anywhere
    bo = _capi.BeamOut(*[buf.data_ptr() if q not in kw.get("skip", ()) else None for q in OWN])
    for q in products:
        setattr(bo.products, PRODUCT_FIELDS[q], buf.data_ptr())
    rc = planner._lib.fpe_plan_beam_device(planner._h, _capi.ptr(planner.params), C.byref(bp), C.c_void_p(d_poses.data_ptr()), None, c["B"],
                                           C.c_void_p(d_options.data_ptr()), kw.get("M", options.shape[0]), C.byref(bo), None)
    torch.cuda.synchronize()
    assert rc == _capi.FPE_E_INVALID_ARG, what
    assert bool((buf == FILL).all())


def test_forced_groups_without_a_resume_kernel_are_refused(planner):
    c = use_case(planner, "w7_gen")
    with planner.tuning(plan_group=4):
        rc, out = host_beam(planner, c["roots"], c["options"], beam_params(c))
        assert rc == _capi.FPE_E_UNSUPPORTED
        assert all(np.all(v.view(np.uint8) == FILL) for v in out.values())
    rc, out = host_beam(planner, c["roots"], c["options"], beam_params(c))  # ... and runs again without the knob
    assert rc == _capi.FPE_OK and (out["n_live"] == c["W"]).all()


def test_packed_bound_applies_only_when_the_product_is_requested(planner):
    """A map of more than FPE_PACKED_MAX_CELLS columns: selected_packed is refused (FPE_E_UNSUPPORTED, nothing written), the same call
    without it runs."""
    c = bref.case("w7_gen")
    planner.params = c["params"].copy()
    planner.set_max_leg_search_radius(0.0)
    cols = _capi.PACKED_MAX_CELLS + 1
    planner.gridmapCallback(np.ones((64, cols), np.float32), np.zeros((64, cols), np.float32), 0.02)
    rc, out = host_beam(planner, c["roots"], c["options"], beam_params(c), products=("selected_packed",))
    assert rc == _capi.FPE_E_UNSUPPORTED and all(np.all(v.view(np.uint8) == FILL) for v in out.values())
    rc, out = host_beam(planner, c["roots"], c["options"], beam_params(c), products=("cycle_ok",))
    assert rc == _capi.FPE_OK and (out["n_live"] == c["W"]).all()


def test_python_wrapper_returns_the_documented_dict(planner):
    c = use_case(planner, "w7_gen")
    w = c["weights"]
    got = planner.plan_beam(c["roots"], c["options"], beam=dict(segments=c["S"], cycles_per_segment=c["k"], width=c["W"], w_fail=w[0], w_spiral=w[1],
                                                               w_none=w[2], w_deviation=w[3], w_progress=w[4]))
    ref = bref.reference("w7_gen")
    assert set(got) == {"path", "score", "penalty", "n_live", "state", "nominal", "cycle_ok"}
    assert got["nominal"].shape == (c["B"], c["W"], c["S"] * c["k"], 4) and got["cycle_ok"].shape == (c["B"], c["W"], c["S"] * c["k"])
    for q in ("path", "score", "penalty", "n_live", "state"):
        assert got[q].tobytes() == np.ascontiguousarray(ref[q]).tobytes(), q
