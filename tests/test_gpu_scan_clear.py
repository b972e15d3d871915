"""Scan visibility clearing on the device (fpe_scan_clear*; include/fpe.h) against the numpy statement of the contract
(tests/scan_clear_reference.py), in every form of the ray pass.  Every comparison is of bits: both layers over the whole state and the
whole info record — and, for the way into the planner's snapshot, both snapshot layers against a second engine that was driven through
the older public entry points only.

The priors differ from cell to cell (sr.prior_layers), so a cell that was written although no ray counted against it shows.  That the
cases hold cells at and just below min_hits, samples over unknown cells, rays that cross a roi they do not end in, rays of more than
64 samples and every per-point counter is asserted of the reference alone in tests/test_cpu_scan_clear.py.  The scan tests' shapes:
maps of 100 x 72 and 48 x 40 at 2 cm, at most 20 000 points."""
import ctypes as C

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, FpeError, make_scan, scan_clear_params, scan_params
from tests import elevation_update_reference as er
from tests import scan_clear_reference as cr
from tests import scan_reference as sr

pytestmark = pytest.mark.gpu

FORMS = {"lane": dict(scan_clear_form=1), "group16": dict(scan_clear_form=2, scan_clear_group=16), "group32": dict(scan_clear_form=2, scan_clear_group=32),
         "group64": dict(scan_clear_form=2, scan_clear_group=64)}
TWO_FORMS = ["lane", "group16"]  # where the case is about something else than the ray pass's lanes


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def cases():
    return sr.fuse_cases()


@pytest.fixture(scope="module")
def states(planner, cases):
    """One state per map geometry of the cases, reused: every test sets both layers first."""
    made = {}

    def get(case):
        key = (case["rows"], case["cols"], case["pos"])
        if key not in made:
            made[key] = planner.scan_state(case["rows"], case["cols"], case["res"], case["pos"])
        return made[key]

    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def reference():
    """cr.run, computed once per key and shared by the forms."""
    memo = {}

    def get(key, case, **kw):
        if key not in memo:
            memo[key] = cr.run(case, **kw)
        return memo[key]

    return get


def sp_struct(p):
    return scan_params(**{k: (int(v) if k == "replace_count" else float(v)) for k, v in p.items()})


def cp_struct(cp):
    return scan_clear_params(**{k: (float(v) if k in cr.FLOAT_FIELDS else int(v)) for k, v in cp.items()})


def device(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(3, np.float32)).cuda()


def n_stride(points):
    return len(points), (points.shape[1] if points.ndim == 2 and len(points) else 3)


def gpu_clear(state, case, cp=None, points=None, roi=None, elev=None, var=None, host=False, set_layers=True):
    """set_layers, one clear (device form unless `host`) -> (elevation, variance, the info's sixteen words)."""
    import torch

    points = case["points"] if points is None else points
    roi = case["roi"] if roi is None else roi
    if set_layers:
        state.set_layers(case["elev"] if elev is None else elev, case["var"] if var is None else var)
    scan = make_scan(case["T"], n_stride(points)[0], roi, n_stride(points)[1])
    sp, cps = sp_struct(case["params"]), cp_struct(cr.params() if cp is None else cp)
    if host:
        words = cr.words(state.clear(scan, points, sp, cps))
    else:
        d_pts = device(points)
        d_info = torch.full((16,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        state.clear_device(scan, d_pts.data_ptr(), sp, cps, d_info.data_ptr())
        torch.cuda.synchronize()
        words = d_info.cpu().numpy()
    e, v = state.read_layers()
    return e, v, words


def gpu_fuse(state, case, points=None, roi=None):
    """One device fuse into the state as it is -> (elevation, variance, info words)."""
    import torch

    points = case["points"] if points is None else points
    d_pts, d_info = device(points), torch.full((16,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    state.fuse_device(make_scan(case["T"], n_stride(points)[0], case["roi"] if roi is None else roi, n_stride(points)[1]), d_pts.data_ptr(),
                      sp_struct(case["params"]), d_info.data_ptr())
    torch.cuda.synchronize()
    return (*state.read_layers(), d_info.cpu().numpy())


def assert_equal(got, want, what):
    """got: (e, v, sixteen words); want: the same, or the reference's (e, v, info record, ...)."""
    (e, v, words), (re, rv, rinfo) = got, want[:3]
    rwords = rinfo if isinstance(rinfo, np.ndarray) and rinfo.dtype == np.int32 else cr.words(rinfo)
    print(what, "info", words.tolist())
    assert words.tolist() == rwords.tolist(), f"{what}: info {words.tolist()} against {rwords.tolist()}"
    de, dv = sr.bits(e) != sr.bits(re), sr.bits(v) != sr.bits(rv)
    assert not de.any(), f"{what}: {int(de.sum())} elevation cells differ, first at {np.argwhere(de)[0].tolist()}"
    assert not dv.any(), f"{what}: {int(dv.sum())} variance cells differ, first at {np.argwhere(dv)[0].tolist()}"


# ---- 1. the cases' own prior, every form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(sr.fuse_cases()))
def test_clear_equals_the_reference_on_every_byte(planner, cases, states, reference, name, form):
    c = cases[name]
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear(states(c), c), reference(name, c), f"{name}, {form}")


@pytest.mark.parametrize("form", list(FORMS))
def test_every_per_point_counter(planner, cases, states, reference, form):
    """ray_stride 3 and a small max_samples: strided-out and dropped points, long and empty rays in one call."""
    c = cases["100x72"]
    cp = cr.params(**cr.EVERY_COUNTER)
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear(states(c), c, cp=cp), reference("every counter", c, cp=cp), f"every counter, {form}")


# ---- 2. the ghost ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_ghost_state(planner, cases, states, reference, form):
    c = cases["100x72"]
    ge, gv = cr.ghost_state(c)
    want = reference("ghost", c, elev=ge, var=gv)
    assert 1 <= want[2]["cells_cleared"] <= 36
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear(states(c), c, elev=ge, var=gv), want, f"ghost, {form}")


def test_default_form_clears_nothing_of_the_state_the_scan_made(planner, cases, states):
    """scan_clear_form 0 (the engine's choice), host form."""
    c = cases["48x40"]
    e, v = cr.own_state(c)
    got = gpu_clear(states(c), c, elev=e, var=v, host=True)
    assert_equal(got, cr.run(c, elev=e, var=v), "own state")
    assert np.array_equal(sr.bits(got[0]), sr.bits(e)) and got[2][7] == 0


# ---- 3. launch edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ray_stride", [1, 2, 3])
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("form", list(FORMS))
def test_launch_edges(planner, cases, states, stride, ray_stride, form):
    """Point counts around a wavefront and a workgroup; min_hits 1, so that the few rays of the small counts clear cells."""
    c = cases["100x72" if stride == 3 else "100x72,stride4"]
    pts = sr.shuffled(c, 77)
    cp = cr.params(min_hits=1, ray_stride=ray_stride)
    cleared = 0
    with planner.tuning(**FORMS[form]):
        for n in (0, 1, 63, 64, 65, 255, 256, 257):
            want = cr.run(c, cp=cp, points=pts[:n])
            cleared += int(want[2]["cells_cleared"])
            assert_equal(gpu_clear(states(c), c, cp=cp, points=pts[:n]), want, f"n = {n}, stride {stride}, ray_stride {ray_stride}, {form}")
    assert cleared > 0


# ---- 4. contention ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["one cell", "one point per cell"])
def test_contention(planner, cases, states, reference, name, form):
    """4 096 rays through the same few cells under the sensor, and one ray to every cell, over a prior that stands above the sensor."""
    c = cases["100x72"]
    pts = sr.contention_cases(c)[name]
    e, v = cr.raised(c)
    cp = cr.params(**cr.CONTENTION)
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear(states(c), c, cp=cp, points=pts, elev=e, var=v), reference(name, c, cp=cp, points=pts, elev=e, var=v), f"{name}, {form}")


# ---- 5. roi ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TWO_FORMS)
@pytest.mark.parametrize("name", list(sr.roi_cases(100, 72)))
def test_roi(planner, cases, states, reference, name, form):
    c = cases["100x72"]
    roi, pts = sr.roi_cases(c["rows"], c["cols"])[name], sr.roi_points(c)
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear(states(c), c, points=pts, roi=roi), reference("roi " + name, c, points=pts, roi=roi), f"{name}, {form}")


@pytest.mark.parametrize("form", TWO_FORMS)
def test_rays_that_end_beyond_the_map(planner, cases, states, reference, form):
    c = cases["100x72"]
    gp, cp = cr.grazing_points(c), cr.params(min_hits=1)
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear(states(c), c, cp=cp, points=gp), reference("grazing", c, cp=cp, points=gp), f"grazing, {form}")


@pytest.mark.parametrize("form", TWO_FORMS)
def test_two_clears_in_a_row_with_different_rois(planner, cases, states, form):
    """Hits the first call left behind would show in the second: the local cell indices of the two rois differ."""
    c = cases["100x72"]
    s = states(c)
    re, rv = c["elev"], c["var"]
    with planner.tuning(**FORMS[form]):
        for k, roi in enumerate(sr.TWO_ROIS):
            pts = c["points"] if k == 0 else sr.shuffled(c, 9)
            want = cr.run(c, points=pts, roi=roi, elev=re, var=rv)
            assert_equal(gpu_clear(s, c, points=pts, roi=roi, elev=re, var=rv, set_layers=k == 0), want, f"clear {k}, {form}")
            re, rv = want[:2]


# ---- 6. arithmetic ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_permuted_points_give_identical_bytes(planner, cases, states, form):
    """GPU against GPU, far from the origin (the yawed and pitched case against the reference: test 1)."""
    c = cases["far,pitched"]
    with planner.tuning(**FORMS[form]):
        a = gpu_clear(states(c), c)
        for seed in (3, 4):
            assert_equal(gpu_clear(states(c), c, points=sr.shuffled(c, seed)), a, f"permutation {seed}, {form}")


# ---- 7. the scratch is at rest after a clear ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TWO_FORMS)
def test_clear_and_fuse_share_the_scratch(planner, cases, states, form):
    c = cases["100x72"]
    s = states(c)
    with planner.tuning(**FORMS[form]):
        # clear -> fuse
        r_clear = cr.run(c)
        assert_equal(gpu_clear(s, c), r_clear, f"clear, {form}")
        r_fuse = sr.run(c, elev=r_clear[0], var=r_clear[1])
        assert r_clear[2]["cells_hit"] > r_clear[2]["cells_cleared"] > 0  # cells with hits below min_hits: their hits must be gone too
        got = gpu_fuse(s, c)
        assert got[2].tolist() == r_fuse[2].tolist(), f"fuse after clear, {form}"
        assert np.array_equal(sr.bits(got[0]), sr.bits(r_fuse[0])) and np.array_equal(sr.bits(got[1]), sr.bits(r_fuse[1])), f"fuse after clear, {form}"
        # fuse -> clear -> fuse, on from there, with other points
        pts = sr.shuffled(c, 12)[:9000]
        r_clear2 = cr.run(c, points=pts, elev=r_fuse[0], var=r_fuse[1])
        assert_equal(gpu_clear(s, c, points=pts, set_layers=False), r_clear2, f"clear after fuse, {form}")
        r_fuse2 = sr.run(c, points=pts, elev=r_clear2[0], var=r_clear2[1])
        got = gpu_fuse(s, c, points=pts)
        assert got[2].tolist() == r_fuse2[2].tolist(), f"second fuse, {form}"
        assert np.array_equal(sr.bits(got[0]), sr.bits(r_fuse2[0])) and np.array_equal(sr.bits(got[1]), sr.bits(r_fuse2[1])), f"second fuse, {form}"


def test_a_clear_that_clears_nothing_changes_no_later_fuse(planner, cases, states):
    """GPU against GPU: the scan's own state, cleared with the same scan (0 cells), fused — against the same state fused at once."""
    c = cases["48x40"]
    s = states(c)
    e, v = cr.own_state(c)
    s.set_layers(e, v)
    plain = gpu_fuse(s, c)
    got = gpu_clear(s, c, elev=e, var=v)
    assert got[2][7] == 0 and got[2][3] > 19000
    after = gpu_fuse(s, c)
    assert after[2].tolist() == plain[2].tolist()
    assert np.array_equal(sr.bits(after[0]), sr.bits(plain[0])) and np.array_equal(sr.bits(after[1]), sr.bits(plain[1]))


# ---- 8. into the planner's snapshot ------------------------------------------------------------------------------------------------------
INGESTS = [((0, 0), (10, 5, 80, 60)), ((5, 3), (0, 0, 100, 72)), ((-7, 0), (30, 14, 41, 37))]  # (shift, roi); the first neither moves nor shifts


def test_install_and_three_ingest_clears_equal_the_public_steps_by_hand(planner):
    """A: install, then ingest_clear_device three times.  B: a second engine that never sees a scan state: uploaded with A's layers behind
    the install, then update_elevation with the state's roi as a host patch.  C: a third engine and state through the HOST form."""
    import torch

    rows, cols, res = 100, 72, sr.RES
    pos = (0.0, 0.0)
    first = sr.main_case("100x72", pos=pos, seed=99)
    cp = cr.params()
    a, b, c = planner, FootholdPlanner(0), FootholdPlanner(0)
    sa, sc = a.scan_state(rows, cols, res, pos), c.scan_state(rows, cols, res, pos)
    try:
        for s in (sa, sc):
            s.set_layers(first["elev"], first["var"])
            s.install()
        re, rv = first["elev"], first["var"]
        ta, ea = a.read_map_layers()
        b.gridmapCallback(ta, ea, res, position=pos)
        cleared_and_new = 0
        for k, (shift, roi) in enumerate(INGESTS):
            pos = er.moved_position(pos, shift, res) if shift != (0, 0) else pos
            case = sr.main_case("100x72", pos=pos, seed=100 + k, width=128, height=96)
            pts = case["points"]
            scan, sp, cps = make_scan(case["T"], len(pts), roi), sp_struct(case["params"]), cp_struct(cp)
            d_pts = device(pts)
            d_cinfo, d_info = (torch.full((16,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            ui_a = sa.ingest_clear_device(scan, d_pts.data_ptr(), shift, pos, sp, cps, d_clear_info_ptr=d_cinfo.data_ptr(), d_info_ptr=d_info.data_ptr())
            torch.cuda.synchronize()
            # the reference: move, clear, fuse
            me, mv = sr.move(re, shift), sr.move(rv, shift)
            ce, cv, cinfo, _ = cr.clear(me, mv, res, pos, case["params"], cp, case["T"], pts, roi)
            re, rv, rinfo, _, cell_cls = sr.fuse(ce, cv, res, pos, case["params"], case["T"], pts, roi)
            se, sv = sa.read_layers()
            assert_equal((se, sv, d_cinfo.cpu().numpy()), (re, rv, cinfo), f"ingest {k}: the state and the clear's info")
            assert d_info.cpu().numpy().tolist() == rinfo.tolist(), f"ingest {k}: the fuse's info"
            gone = (~np.isnan(me) & np.isnan(ce))[roi[0]:roi[0] + roi[2], roi[1]:roi[1] + roi[3]].reshape(-1)
            cleared_and_new += int((gone & (cell_cls == 1)).sum())
            ta, ea = a.read_map_layers()
            assert np.array_equal(sr.bits(ea), sr.bits(se)), f"ingest {k}: the snapshot's elevation is not the state's"
            # B, by hand: the state's roi read back, one host patch
            r0, c0, nr, nc = roi
            ui_b = b.update_elevation(shift, pos, [(r0, c0, se[r0:r0 + nr, c0:c0 + nc])])
            tb, eb = b.read_map_layers()
            assert ui_a == ui_b and a.map_info() == b.map_info(), f"ingest {k}"
            assert np.array_equal(sr.bits(ea), sr.bits(eb)) and np.array_equal(sr.bits(ta), sr.bits(tb)), f"ingest {k}: A and B differ"
            # C: the host form
            cinfo_c, info_c, ui_c = sc.ingest_clear(scan, pts, shift, pos, sp, cps)
            tc, ec = c.read_map_layers()
            assert ui_c == ui_a and cr.words(cinfo_c).tolist() == cr.words(cinfo).tolist() and cr.words(info_c).tolist() == rinfo.tolist()
            assert np.array_equal(sr.bits(ec), sr.bits(ea)) and np.array_equal(sr.bits(tc), sr.bits(ta)), f"ingest {k}: host and device forms differ"
            he, hv = sc.read_layers()
            assert np.array_equal(sr.bits(he), sr.bits(se)) and np.array_equal(sr.bits(hv), sr.bits(sv))
            assert k > 0 or cinfo["cells_cleared"] > 0
        assert cleared_and_new > 0  # cells that were cleared and hit by the same scan came out NEW
    finally:
        sa.close()
        sc.close()
        b.close()
        c.close()


def test_host_forms_equal_device_forms(planner, cases, states):
    c = cases["48x40"]
    s = states(c)
    assert_equal(gpu_clear(s, c, host=True), gpu_clear(s, c), "clear, host against device")
    # a null info is allowed in both forms
    s.set_layers(c["elev"], c["var"])
    scan, sp, cps = make_scan(c["T"], len(c["points"]), c["roi"]), sp_struct(c["params"]), cp_struct(cr.params())
    assert planner._lib.fpe_scan_clear(s._s, C.byref(sp), C.byref(cps), C.byref(scan), c["points"].ctypes.data_as(C.c_void_p), None) == _capi.FPE_OK
    e, v = s.read_layers()
    want = cr.run(c)
    assert np.array_equal(sr.bits(e), sr.bits(want[0])) and np.array_equal(sr.bits(v), sr.bits(want[1]))
    assert_equal(gpu_clear(s, c), want, "after a call without an info")


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_and_the_snapshot_unchanged(planner, cases):
    import torch

    c = cases["48x40"]
    rows, cols, res, pos = c["rows"], c["cols"], c["res"], c["pos"]
    L = planner._lib
    s = planner.scan_state(rows, cols, res, pos)
    try:
        s.set_layers(c["elev"], c["var"])
        s.install()
        e0, v0 = s.read_layers()
        t0, m0 = planner.read_map_layers()
        d_pts = device(c["points"])
        torch.cuda.synchronize()
        good, sp, cp = make_scan(c["T"], len(c["points"]), c["roi"]), sp_struct(c["params"]), scan_clear_params()

        def refused(call, what):
            with pytest.raises(FpeError) as ei:
                call()
            assert ei.value.code == _capi.FPE_E_INVALID_ARG, what
            torch.cuda.synchronize()
            e, v = s.read_layers()
            t, m = planner.read_map_layers()
            assert np.array_equal(sr.bits(e), sr.bits(e0)) and np.array_equal(sr.bits(v), sr.bits(v0)), what
            assert np.array_equal(sr.bits(t), sr.bits(t0)) and np.array_equal(sr.bits(m), sr.bits(m0)), what
            assert s.geometry()["position"] == pos and planner.map_info()["position"] == pos, what

        bad_cps = {"sample_step 0": dict(sample_step=0.0), "sample_step 2": dict(sample_step=2.0), "NaN margin": dict(margin=np.nan),
                   "negative margin": dict(margin=-0.1), "start_samples -1": dict(start_samples=-1), "end_samples -1": dict(end_samples=-1),
                   "min_hits 0": dict(min_hits=0), "ray_stride 0": dict(ray_stride=0), "max_samples 0": dict(max_samples=0),
                   "max_samples 65537": dict(max_samples=65537), "reserved": dict(reserved=7)}
        for what, kw in bad_cps.items():
            bad = scan_clear_params(**kw)
            refused(lambda: s.clear_device(good, d_pts.data_ptr(), sp, bad), what)
            refused(lambda: s.clear(good, c["points"], sp, bad), what + ", host")
            refused(lambda: s.ingest_clear_device(good, d_pts.data_ptr(), (1, 1), (0.5, 0.5), sp, bad), what + ", ingest")
            refused(lambda: s.ingest_clear(good, c["points"], (1, 1), (0.5, 0.5), sp, bad), what + ", ingest, host")
        bad_scans = {"stride 2": make_scan(c["T"], 10, c["roi"], point_stride=2), "n_points -1": make_scan(c["T"], -1, c["roi"]),
                     "empty roi": make_scan(c["T"], 10, (0, 0, 0, 5)), "roi outside": make_scan(c["T"], 10, (40, 0, 9, 5)),
                     "non-finite transform": make_scan(np.where(np.arange(12) == 3, np.nan, c["T"]), 10, c["roi"])}
        for what, scan in bad_scans.items():
            refused(lambda: s.clear_device(scan, d_pts.data_ptr(), sp, cp), what)
            refused(lambda: s.ingest_clear_device(scan, d_pts.data_ptr(), (1, 1), (0.5, 0.5), sp, cp), what + ", ingest")
        for what, kw in {"gate 0": dict(gate=0.0), "min_z above max_z": dict(min_z=1.0, max_z=0.0), "NaN band": dict(band=np.nan)}.items():
            bad = scan_params(**kw)
            refused(lambda: s.clear_device(good, d_pts.data_ptr(), bad, cp), what)
            refused(lambda: s.ingest_clear(good, c["points"], (1, 1), (0.5, 0.5), bad, cp), what + ", ingest")
        refused(lambda: s.ingest_clear_device(good, d_pts.data_ptr(), (1, 0), (np.inf, 0.0), sp, cp), "ingest at an infinite position")
        refused(lambda: s.ingest_clear_device(good, d_pts.data_ptr(), (0, 0), pos, sp, cp, filter_params=planner.filter_params(normal_radius=-1.0)),
                "ingest with a bad filter radius")
        # null arguments, straight through ctypes
        p = C.c_void_p(d_pts.data_ptr())
        sh, ps = (C.c_int32 * 2)(0, 0), (C.c_double * 2)(*pos)
        null = [L.fpe_scan_clear_device(s._s, C.byref(sp), None, C.byref(good), p, None, None),
                L.fpe_scan_clear_device(s._s, None, C.byref(cp), C.byref(good), p, None, None),
                L.fpe_scan_clear_device(s._s, C.byref(sp), C.byref(cp), None, p, None, None),
                L.fpe_scan_clear_device(s._s, C.byref(sp), C.byref(cp), C.byref(good), None, None, None),
                L.fpe_scan_clear_device(None, C.byref(sp), C.byref(cp), C.byref(good), p, None, None),
                L.fpe_scan_clear(s._s, C.byref(sp), C.byref(cp), C.byref(good), None, None),
                L.fpe_scan_ingest_clear_device(planner._h, s._s, None, C.byref(sp), None, C.byref(good), p, sh, ps, None, None, None, None),
                L.fpe_scan_ingest_clear_device(planner._h, s._s, None, C.byref(sp), C.byref(cp), C.byref(good), p, None, ps, None, None, None, None),
                L.fpe_scan_ingest_clear_device(None, s._s, None, C.byref(sp), C.byref(cp), C.byref(good), p, sh, ps, None, None, None, None)]
        assert null == [_capi.FPE_E_INVALID_ARG] * len(null)
        refused(lambda: planner.set_tuning(scan_clear_form=3), "scan_clear_form 3")
        refused(lambda: planner.set_tuning(scan_clear_group=8), "scan_clear_group 8")
        planner.set_tuning(scan_clear_form=0, scan_clear_group=0)
        # and a valid call with every info null goes through: the state changes, the snapshot follows
        assert L.fpe_scan_ingest_clear_device(planner._h, s._s, None, C.byref(sp), C.byref(cp), C.byref(good), p, sh, ps, None, None, None, None) == _capi.FPE_OK
        torch.cuda.synchronize()
        ce, cv = cr.run(c)[:2]
        want = sr.run(c, elev=ce, var=cv)
        e, v = s.read_layers()
        assert np.array_equal(sr.bits(e), sr.bits(want[0])) and np.array_equal(sr.bits(v), sr.bits(want[1]))
        assert np.array_equal(sr.bits(planner.read_map_layers()[1]), sr.bits(e))
    finally:
        s.close()
