"""The checked beam on the GPU (fpe_plan_beam_checked*; include/fpe.h): both forms against the helper of
tests/beam_checked_reference.py — path, n_live, penalty, base_penalty, score, state, hit, feet, the three summaries and every product,
byte for byte — and against UNCHANGED engine code: fpe_check_plan_device on the final slots' products (the contract),
fpe_plan_resume (the replay) and fpe_plan_beam (no check enabled).  Bytes and integers only, no tolerance anywhere.  Every call
writes into sentinel-filled buffers: dead slots and the outputs of disabled checks must keep the sentinel.  That the inputs hold
what the feature adds is asserted on the helper alone in tests/test_cpu_beam_checked.py."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import PRODUCT_FIELDS, FootholdPlanner, FpeError, make_check_params
from tests import beam_checked_reference as bcref
from tests import beam_reference as bref
from tests import margin_reference
from tests import rank_checked_reference as cref
from tests import resume_reference as rref
from tests import test_gpu_beam as tgb
from tests import test_gpu_rank_checked as tgr

pytestmark = pytest.mark.gpu

PRODUCTS = FootholdPlanner.BEAM_PRODUCTS
FILL = tgb.FILL
CHECK_OWN = {"swing": (_capi.SWING_SUMMARY_DTYPE, ()), "trunk": (_capi.TRUNK_SUMMARY_DTYPE, ()), "margin": (_capi.MARGIN_SUMMARY_DTYPE, ()),
             "base_penalty": (np.dtype(np.float64), ()), "hit": (np.dtype(np.uint8), ()), "feet": (np.dtype(np.float64), (4, 3))}
BITS = {"swing": cref.SWING, "trunk": cref.TRUNK, "margin": cref.MARGIN}


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.set_max_leg_search_radius(0.0)
    p.close()


def use_case(planner, name):
    c = bcref.base_case(name)
    planner.params = c["params"].copy()
    planner.set_max_leg_search_radius(float(c["row"].maxleg or 0.0))
    planner.gridmapCallback(c["trav"], c["elev"], c["row"].res)
    return c


def check_shapes(B, W):
    return {q: ((B, W) + tail, dt) for q, (dt, tail) in CHECK_OWN.items()}


def view(raw, shapes):
    return {q: raw[q].view(shapes[q][1]).reshape(shapes[q][0]) for q in raw}


def host_checked(planner, c, checks, feet="case", states="case", products=PRODUCTS, bp=None, want=tuple(CHECK_OWN), name=None, skip=(),
                 shape=None, M=None):
    """fpe_plan_beam_checked through the C ABI into sentinel-filled arrays: (status, beam outputs, check outputs) as typed views
    (shape: the (S, k, W) the buffers are sized for where the parameters' own are refused; M: the option count passed)"""
    bp = bp or tgb.beam_params(c)
    S, k, W = shape or (bp.segments, bp.cycles_per_segment, bp.width)
    B = c["roots"].shape[0]
    shapes, cshapes = tgb.out_shapes(B, W, S, k, products), check_shapes(B, W)
    raw = {q: np.full(tgb.nbytes(*shapes[q]), FILL, np.uint8) for q in shapes}
    craw = {q: np.full(tgb.nbytes(*cshapes[q]), FILL, np.uint8) for q in cshapes}
    bo = tgb.beam_out({q: _capi.ptr(raw[q]) for q in raw}, products, skip)
    co = _capi.BeamCheckOut(**{q: _capi.ptr(craw[q]) for q in want})
    feet = bcref.start_feet(name or c["name"]) if isinstance(feet, str) else feet
    states = c["states"] if isinstance(states, str) else states
    cp = checks if isinstance(checks, _capi.CheckParams) or checks is None else cref.make_engine_params(checks)
    rc = planner._lib.fpe_plan_beam_checked(planner._h, _capi.ptr(planner.params), C.byref(bp), C.byref(cp) if cp is not None else None,
                                            _capi.ptr(c["roots"]), _capi.ptr(states), _capi.ptr(np.ascontiguousarray(feet)) if feet is not None else None,
                                            B, _capi.ptr(c["options"]), c["options"].shape[0] if M is None else M, C.byref(bo), C.byref(co))
    return rc, view(raw, shapes), view(craw, cshapes)


def device_checked(planner, c, checks, feet="case", states="case", products=PRODUCTS, bp=None, want=tuple(CHECK_OWN), name=None, after_queue=None):
    """fpe_plan_beam_checked_device on a stream of its own into sentinel-filled device buffers (after_queue: called while it is queued)"""
    bp = bp or tgb.beam_params(c)
    B, W = c["roots"].shape[0], bp.width
    shapes, cshapes = tgb.out_shapes(B, W, bp.segments, bp.cycles_per_segment, products), check_shapes(B, W)
    feet = bcref.start_feet(name or c["name"]) if isinstance(feet, str) else feet
    states = c["states"] if isinstance(states, str) else states
    d_poses, d_options = tgr.dev(c["roots"]), tgr.dev(c["options"])
    d_states = tgr.dev(states) if states is not None else None
    d_feet = tgr.dev(feet) if feet is not None else None
    raw = {q: torch.full((tgb.nbytes(*shapes[q]),), FILL, dtype=torch.uint8, device="cuda") for q in shapes}
    craw = {q: torch.full((tgb.nbytes(*cshapes[q]),), FILL, dtype=torch.uint8, device="cuda") for q in cshapes}
    cp = checks if isinstance(checks, _capi.CheckParams) or checks is None else cref.make_engine_params(checks)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        planner.plan_beam_checked_device(d_poses.data_ptr(), B, d_options.data_ptr(), c["options"].shape[0], raw["path"].data_ptr(), beam=bp,
                                         checks=cp, d_state_in_ptr=d_states.data_ptr() if d_states is not None else 0,
                                         d_start_feet_ptr=d_feet.data_ptr() if d_feet is not None else 0, d_n_live_ptr=raw["n_live"].data_ptr(),
                                         d_score_ptr=raw["score"].data_ptr(), d_penalty_ptr=raw["penalty"].data_ptr(),
                                         d_state_ptr=raw["state"].data_ptr(), products={q: raw[q].data_ptr() for q in products},
                                         check_out={q: craw[q].data_ptr() for q in want}, stream=stream.cuda_stream)
        if after_queue:
            after_queue()
    stream.synchronize()
    return view({q: t.cpu().numpy() for q, t in raw.items()}, shapes), view({q: t.cpu().numpy() for q, t in craw.items()}, cshapes)


def run_form(planner, form, c, checks, **kw):
    if form == "device":
        return device_checked(planner, c, checks, **kw)
    rc, got, cgot = host_checked(planner, c, checks, **kw)
    assert rc == _capi.FPE_OK, planner._lib.fpe_last_error(planner._h)
    return got, cgot


def untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


def assert_checked_is(got, cgot, ref, on, products, what, nan_equal=False):
    """The beam's outputs as tests/test_gpu_beam.py compares them, then the check outputs: live slots equal the helper's byte for
    byte, dead slots and the summaries of disabled checks hold the sentinel."""
    tgb.assert_beam_is(got, ref, products, what, nan_equal)
    n = int(ref["n_live"][0])
    want = {"base_penalty": ref["base_penalty"], "hit": ref["hit"], "feet": ref["feet"]}
    want.update({q: ref["sums"][q] for q in BITS if on & BITS[q]})
    for q in CHECK_OWN:
        if q not in want:
            assert untouched(cgot[q]), f"{what}: the output of the disabled check {q} was written"
            continue
        live, dead = cgot[q][:, :n], cgot[q][:, n:]
        if not tgb.same_bits(live, want[q], nan_equal):
            bad = [(b, s) for b in range(live.shape[0]) for s in range(n) if not tgb.same_bits(live[b, s], want[q][b, s], nan_equal)]
            raise AssertionError(f"{what}: {q} differs in {len(bad)} live slots, first (root, slot) {bad[0]}: {live[bad[0]]!r} vs {want[q][bad[0]]!r}")
        assert untouched(dead), f"{what}: a dead slot of {q} was written"


# ---- 1. parity with the helper, both forms, every case -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", [n for n in bcref.CASES if n != "nan_option"])
def test_checked_beam_is_the_helpers(planner, name, form):
    c = use_case(planner, name)
    products = ("nominal", "cycle_ok") if name == "largest_sort" else PRODUCTS
    feet = None if name == "stance_start" else "case"
    got, cgot = run_form(planner, form, c, bcref.checks_of(name), feet=feet, products=products, name=name)
    assert_checked_is(got, cgot, bcref.reference(name), 7, products, f"{name}, {form} form")


def test_device_form_puts_non_finite_candidates_in_class_2_by_index(planner):
    c = use_case(planner, "nan_option")
    got, cgot = device_checked(planner, c, bcref.checks_of("nan_option"))
    assert np.isfinite(got["score"][:, :12]).all() and np.isnan(got["score"][:, 12:]).all()
    assert got["path"][:, 12:].tolist() == [[[1, m] for m in range(4)]] * c["B"]
    assert_checked_is(got, cgot, bcref.reference("nan_option"), 7, PRODUCTS, "NaN option", nan_equal=True)
    rc, out, cout = host_checked(planner, c, bcref.checks_of("nan_option"))   # the host form looks at the values
    assert rc == _capi.FPE_E_INVALID_ARG and all(untouched(v) for v in list(out.values()) + list(cout.values()))


# ---- 2. the contract against unchanged code --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w7_gen", "w7_gen_k5", "w16_seq", "w48_raised", "underfilled", "resumed", "stance_start"])
def test_final_slots_are_what_the_check_stage_writes_for_their_products(planner, name):
    """fpe_check_plan_device — code this feature does not touch — on the live slots' nominal and cycle_ok, S * k cycles, with the
    roots' start feet: its summaries and hit are the checked beam's, byte for byte."""
    c = use_case(planner, name)
    checks = bcref.checks_of(name)
    got, cgot = run_form(planner, "device", c, checks, feet=None if name == "stance_start" else "case", name=name)
    n = int(got["n_live"][0])
    B, cycles = c["B"], c["S"] * c["k"]
    nominal, ok = np.ascontiguousarray(got["nominal"][:, :n]), np.ascontiguousarray(got["cycle_ok"][:, :n])
    feet = np.ascontiguousarray(np.repeat(bcref.start_feet(name), n, axis=0))
    d = {"nominal": tgr.dev(nominal), "cycle_ok": tgr.dev(ok), "feet": tgr.dev(feet), "stance": tgr.dev(feet)}
    want = tgr.run_stage(planner, d, B * n, cycles, checks, True)
    for q in ("swing", "trunk", "margin", "hit"):
        assert np.ascontiguousarray(cgot[q][:, :n]).tobytes() == want[q].tobytes(), (name, q)


@pytest.mark.parametrize("name", ["w7_gen", "w16_seq", "resumed"])
def test_replaying_every_slots_path_with_plan_resume_gives_its_products_state_and_feet(planner, name):
    c = use_case(planner, name)
    got, cgot = run_form(planner, "host", c, bcref.checks_of(name), name=name)
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
    feet = bcref.start_feet(name)
    for b, w in itertools.product(range(B), range(W)):
        assert np.array_equal(cgot["feet"][b, w], bcref.carried_feet(got["nominal"][b, w], got["cycle_ok"][b, w], feet[b]))


# ---- 3. subsets of the checks, reject sets, reaches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", range(1, 8))
def test_every_subset_of_the_checks_leaves_the_disabled_outputs_alone(planner, on):
    c = use_case(planner, "w7_gen")
    checks = bcref.checks_of("w7_gen", checks=on, reject=bcref.REJECT & on)
    ref = bcref.run("w7_gen", checks)
    for form in ("host", "device"):
        got, cgot = run_form(planner, form, c, checks)
        assert_checked_is(got, cgot, ref, on, PRODUCTS, f"checks {on}, {form} form")


@pytest.mark.parametrize("form", ["host", "device"])
def test_without_checks_every_byte_is_the_unchecked_beams_and_check_out_is_untouched(planner, form):
    c = use_case(planner, "w7_gen")
    got, cgot = run_form(planner, form, c, dict(checks=0))
    want = tgb.run_form(planner, form, c, tgb.beam_params(c))
    for q in want:
        assert np.ascontiguousarray(got[q]).tobytes() == np.ascontiguousarray(want[q]).tobytes(), q
    assert all(untouched(v) for v in cgot.values())
    tgb.assert_beam_is(got, bref.reference("w7_gen"), PRODUCTS, f"no checks, {form} form")


@pytest.mark.parametrize("reject", [0, 1, 2, 4, 8, 15])
def test_reject_sets(planner, reject):
    c = use_case(planner, "underfilled")
    checks = bcref.checks_of("underfilled", reject=reject)
    ref = bcref.run("underfilled", checks)
    got, cgot = run_form(planner, "device", c, checks)
    assert_checked_is(got, cgot, ref, 7, PRODUCTS, f"reject {reject}")
    if reject == 0:
        assert all(set(sg["classes"]) == {0} for root in ref["log"] for sg in root)


@pytest.mark.parametrize("reach", [1, 8, 31])   # lanes per cell of the margin: 4, 4 (five rounds), 64
def test_margin_reaches(planner, reach):
    c = use_case(planner, "underfilled")
    checks = bcref.checks_of("underfilled", checks=cref.MARGIN, reject=cref.MARGIN,
                             margin=dict(classes=13, reach_cells=reach, min_margin=0.5 * c["row"].res))
    ref = bcref.run("underfilled", checks)
    got, cgot = run_form(planner, "device", c, checks)
    assert_checked_is(got, cgot, ref, cref.MARGIN, PRODUCTS, f"reach {reach}")
    assert ref["sums"]["margin"]["n_footholds"].sum() > 0


@pytest.mark.parametrize("waves", [1, 4])
def test_the_lane_mapping_of_the_check_kernel_changes_no_byte(planner, waves):
    """One and four wavefronts per candidate (fpe_set_tuning "beam_check_waves"; 0 lets the engine choose by the map's resolution):
    every summary field is a count, an extremum or an argmin with a tie rule, so any dealing of the records to the lanes gives the
    same bytes — at k = 2, where three of four wavefronts have little to do, and at k = 5, where the trunk's chunks wrap."""
    for name in ("w7_gen", "w7_gen_k5"):
        c = use_case(planner, name)
        with planner.tuning(beam_check_waves=waves):
            got, cgot = device_checked(planner, c, bcref.checks_of(name))
        assert_checked_is(got, cgot, bcref.reference(name), 7, PRODUCTS, f"{name}, {waves} wavefronts per candidate")
    with pytest.raises(FpeError) as e:
        planner.set_tuning(beam_check_waves=2)
    assert e.value.code == _capi.FPE_E_INVALID_ARG


# ---- 4. shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_one_option_one_slot(planner, form):
    c = use_case(planner, "degenerate")
    checks = bcref.checks_of("degenerate")
    got, cgot = run_form(planner, form, c, checks)
    assert got["n_live"].tolist() == [1] * c["B"] and not got["path"].any()
    assert_checked_is(got, cgot, bcref.run("degenerate", checks), 7, PRODUCTS, f"degenerate, {form} form")


@pytest.mark.parametrize("form", ["host", "device"])
def test_roots_continued_from_the_state_and_feet_of_a_first_call(planner, form):
    """The best slot of every root of a first call — out.state and check_out.feet — as state_in and start_feet of a second one"""
    c = use_case(planner, "w16_seq")
    checks = bcref.checks_of("w16_seq")
    first, cfirst = run_form(planner, form, c, checks)
    ref1 = bcref.reference("w16_seq")
    states, feet = np.ascontiguousarray(first["state"][:, 0]), np.ascontiguousarray(cfirst["feet"][:, 0])
    assert states.tobytes() == np.ascontiguousarray(ref1["state"][:, 0]).tobytes() and feet.tobytes() == np.ascontiguousarray(ref1["feet"][:, 0]).tobytes()
    got, cgot = run_form(planner, form, c, checks, feet=feet, states=states)
    ref2 = bcref.run("w16_seq", checks, feet=feet, states=states)
    assert_checked_is(got, cgot, ref2, 7, PRODUCTS, f"continued, {form} form")
    assert (got["state"]["cycle"] == 2 * c["S"] * c["k"]).all() and (got["nominal"]["gait_cycle_id"][:, :, 0] == c["S"] * c["k"]).all()
    firsts = np.concatenate([cgot["swing"]["first_over_cycle"].ravel(), cgot["trunk"]["first_bad_cycle"].ravel(), cgot["margin"]["min_cycle"].ravel()])
    assert ((firsts < c["S"] * c["k"]) | (firsts == 255)).all()   # cycle indices count from THIS beam's first cycle


# ---- 5. the snapshot a call sees ---------------------------------------------------------------------------------------------------------
def test_a_call_queued_before_a_second_upload_sees_the_first_snapshot(planner):
    c = use_case(planner, "w7_gen")
    r = rref.case("w7_gen")
    checks = bcref.checks_of("w7_gen")
    got, cgot = device_checked(planner, c, checks, after_queue=lambda: planner.gridmapCallback(r["trav2"], r["elev2"], c["row"].res))
    assert_checked_is(got, cgot, bcref.reference("w7_gen"), 7, PRODUCTS, "the call queued before the upload")
    again, cagain = device_checked(planner, c, checks)   # ... and a call behind the upload sees the second map
    assert again["nominal"].tobytes() != got["nominal"].tobytes()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(planner):
    c = use_case(planner, "resumed")
    assert margin_reference.undecidable(0.1601, 8, c["row"].res)   # (bad_blocks' undecidable min_margin is undecidable on this map too)
    good = bcref.checks_of("resumed")
    inv = _capi.FPE_E_INVALID_ARG

    def host(checks, case=c, **kw):
        rc, out, cout = host_checked(planner, case, checks, name="resumed", **kw)
        assert all(untouched(v) for v in list(out.values()) + list(cout.values())), "a refused host call wrote something"
        return rc

    buf = torch.full((1 << 18,), FILL, dtype=torch.uint8, device="cuda")   # every device pointer: nothing may be written anywhere
    p = buf.data_ptr()
    d_poses, d_options, d_states = tgr.dev(c["roots"]), tgr.dev(c["options"]), tgr.dev(c["states"])

    def device(checks, bp=None, states=True, feet=True, path=True, products=("nominal",)):
        cp = checks if isinstance(checks, _capi.CheckParams) else cref.make_engine_params(checks)
        try:
            planner.plan_beam_checked_device(d_poses.data_ptr(), c["B"], d_options.data_ptr(), c["M"], p if path else 0, beam=bp or tgb.beam_params(c),
                                             checks=cp, d_state_in_ptr=d_states.data_ptr() if states else 0, d_start_feet_ptr=p + 4096 if feet else 0,
                                             d_score_ptr=p + 8192, products={q: p + 16384 for q in products},
                                             check_out={q: p + 65536 + 4096 * k for k, q in enumerate(CHECK_OWN)})
        except FpeError as e:
            return e.code
        return _capi.FPE_OK

    # the check block's own rules, decided by the checked ranking's host functions
    for what, cp, code in tgr.bad_blocks():
        assert host(cp) == code, what
        assert device(cp) == code, what
    # the missing start feet: a swing check from state_in needs them; without the swing, or from the poses, they may be NULL
    assert host(good, feet=None) == inv and device(good, feet=False) == inv
    # the host form looks at the start feet
    for bad in (np.nan, np.inf, 1.5e6):
        feet = bcref.start_feet("resumed").copy()
        feet[1, 2, 1] = bad
        assert host(good, feet=feet) == inv, bad
    # everything fpe_plan_beam refuses
    for what in ("M_17", "W_65", "S_times_k_256", "reserved", "nan_weight", "no_path", "stance", "nan_pose", "inf_option", "nan_state",
                 "cycle_past_255"):
        bp, poses, options, states, products, kw = tgb.refusal_args(c, what)
        assert host(good, case=dict(c, roots=poses, options=options), bp=bp, states=c["states"] if states is None else states,
                    products=products, **kw) == inv, what
        if what in ("W_65", "S_times_k_256", "reserved", "nan_weight", "no_path", "stance"):   # (the device form cannot look at values)
            assert device(good, bp=bp, path=what != "no_path", products=("nominal", "stance") if what == "stance" else ("nominal",)) == inv, what
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()), "a refused device call wrote something"
    # what is NOT refused: no swing -> no start feet needed; from the poses -> the stance
    rc, out, cout = host_checked(planner, c, dict(good, checks=6, reject=2), feet=None)
    assert rc == _capi.FPE_OK and (out["n_live"] == c["W"]).all() and untouched(cout["swing"]) and not untouched(cout["trunk"])
    rc, out, cout = host_checked(planner, c, good, feet=None, states=None)
    assert rc == _capi.FPE_OK and not untouched(cout["swing"])


def test_forced_groups_without_a_resume_kernel_and_a_missing_map_are_refused(planner):
    c = use_case(planner, "w7_gen")
    with planner.tuning(plan_group=4):
        rc, out, cout = host_checked(planner, c, bcref.checks_of("w7_gen"))
        assert rc == _capi.FPE_E_UNSUPPORTED and all(untouched(v) for v in list(out.values()) + list(cout.values()))
    fresh = FootholdPlanner(0)
    try:
        fresh.params = c["params"].copy()
        rc, out, cout = host_checked(fresh, c, bcref.checks_of("w7_gen"))
        assert rc == _capi.FPE_E_NO_MAP and all(untouched(v) for v in list(out.values()) + list(cout.values()))
    finally:
        fresh.close()


def test_python_wrapper_returns_the_documented_dict(planner):
    c = use_case(planner, "w7_gen")
    w = c["weights"]
    checks = bcref.checks_of("w7_gen")
    got = planner.plan_beam_checked(c["roots"], c["options"], beam=dict(segments=c["S"], cycles_per_segment=c["k"], width=c["W"], w_fail=w[0],
                                                                       w_spiral=w[1], w_none=w[2], w_deviation=w[3], w_progress=w[4]),
                                    checks=cref.make_engine_params(checks), start_feet=bcref.start_feet("w7_gen"))
    ref = bcref.reference("w7_gen")
    assert set(got) == {"path", "score", "penalty", "n_live", "state", "nominal", "cycle_ok", "base_penalty", "hit", "feet", "swing_summary",
                        "trunk_summary", "margin_summary"}
    for q in ("path", "score", "penalty", "n_live", "state", "base_penalty", "hit", "feet"):
        assert got[q].tobytes() == np.ascontiguousarray(ref[q]).tobytes(), q
    for q in BITS:
        assert got[q + "_summary"].tobytes() == ref["sums"][q].tobytes(), q
    plain = planner.plan_beam_checked(c["roots"], c["options"], beam=tgb.beam_params(c), checks=make_check_params(checks=0))
    assert set(plain) == {"path", "score", "penalty", "n_live", "state", "nominal", "cycle_ok"}
