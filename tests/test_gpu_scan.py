"""Scan fusion on the device (fpe_scan_*; include/fpe.h) against the numpy statement of the contract (tests/scan_reference.py).
Every comparison is of bits: both layers, all sixteen info words, and — for the way into the planner's snapshot — both snapshot
layers against a second engine that was driven through the older public entry points only.

The priors differ from cell to cell (sr.prior_layers), so a cell that was written although no point fell into it shows.  That each
case holds cells of every class, points of every drop class, a cell with more than 64 kept points and points below the band is
asserted of the reference alone in tests/test_cpu_scan.py.  Maps of 100 x 72 and 48 x 40 at 2 cm (the elevation-update tests'
shapes), scans of at most 20 000 points."""
import ctypes as C

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, FpeError, make_scan, scan_params
from tests import elevation_update_reference as er
from tests import scan_reference as sr

pytestmark = pytest.mark.gpu

MERGE_FORMS = {"plain": 1, "merged": 2}


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


def to_struct(p):
    return scan_params(**{k: (int(v) if k == "replace_count" else float(v)) for k, v in p.items()})


def device(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(3, np.float32)).cuda()


def gpu_fuse(state, case, points=None, roi=None, elev=None, var=None, host=False):
    """set_layers, one fuse (device form unless `host`) -> (elevation, variance, info words)."""
    import torch

    points = case["points"] if points is None else points
    roi = case["roi"] if roi is None else roi
    state.set_layers(case["elev"] if elev is None else elev, case["var"] if var is None else var)
    scan = make_scan(case["T"], len(points), roi, points.shape[1] if points.ndim == 2 and len(points) else 3)
    sp = to_struct(case["params"])
    if host:
        info = state.fuse(scan, points, sp)
        words = np.frombuffer(info.tobytes(), np.int32)
    else:
        d_pts = device(points)
        d_info = torch.full((16,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        state.fuse_device(scan, d_pts.data_ptr(), sp, d_info.data_ptr())
        torch.cuda.synchronize()
        words = d_info.cpu().numpy()
    e, v = state.read_layers()
    return e, v, words


def assert_fuse_equal(got, want, what):
    (e, v, info), (re, rv, rinfo) = got, want[:3]
    print(what, "info", info.tolist())
    assert info.tolist() == rinfo.tolist(), f"{what}: info {dict(zip(sr.INFO_FIELDS, info.tolist()))} bbox {info[12:].tolist()}"
    de, dv = sr.bits(e) != sr.bits(re), sr.bits(v) != sr.bits(rv)
    assert not de.any(), f"{what}: {int(de.sum())} elevation cells differ, first at {np.argwhere(de)[0].tolist()}"
    assert not dv.any(), f"{what}: {int(dv.sum())} variance cells differ, first at {np.argwhere(dv)[0].tolist()}"


# ---- 1. the fuse against the reference, both forms of the point passes ----------------------------------------------------------------
@pytest.mark.parametrize("form", list(MERGE_FORMS))
@pytest.mark.parametrize("name", list(sr.fuse_cases()))
def test_fuse_equals_the_reference_on_every_byte(planner, cases, states, name, form):
    c = cases[name]
    with planner.tuning(scan_merge=MERGE_FORMS[form]):
        assert_fuse_equal(gpu_fuse(states(c), c), sr.run(c), f"{name}, {form}")


def test_default_form_and_unknown_start(planner, cases, states):
    """scan_merge 0 (the engine's choice), into a state nobody has set: every touched cell is NEW."""
    c = cases["48x40"]
    s = planner.scan_state(c["rows"], c["cols"], c["res"], c["pos"])
    try:
        e0, v0 = s.read_layers()
        assert (sr.bits(e0) == sr.CLEARED).all() and (sr.bits(v0) == sr.CLEARED).all()
        assert s.geometry() == {"rows": c["rows"], "cols": c["cols"], "resolution": c["res"], "position": c["pos"]}
        info = s.fuse(make_scan(c["T"], len(c["points"]), c["roi"]), c["points"], to_struct(c["params"]))
        e, v = s.read_layers()
        re, rv, rinfo = sr.fuse(e0, v0, c["res"], c["pos"], c["params"], c["T"], c["points"], c["roi"])[:3]
        assert_fuse_equal((e, v, np.frombuffer(info.tobytes(), np.int32)), (re, rv, rinfo), "unknown start")
        assert info["cells_new"] == info["cells_touched"] > 0
    finally:
        s.close()


# ---- 2. launch edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("form", list(MERGE_FORMS))
def test_launch_edges(planner, cases, states, stride, form):
    """Point counts around a wavefront, a workgroup (256) and two workgroups, with the points of every class among the first."""
    c = cases["100x72" if stride == 3 else "100x72,stride4"]
    pts = sr.shuffled(c, 77)
    with planner.tuning(scan_merge=MERGE_FORMS[form]):
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513):
            assert_fuse_equal(gpu_fuse(states(c), c, points=pts[:n]), sr.run(c, points=pts[:n]), f"n = {n}, stride {stride}, {form}")


# ---- 3. contention -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(MERGE_FORMS))
@pytest.mark.parametrize("name", ["one cell", "one row", "one point per cell"])
def test_contention(planner, cases, states, name, form):
    c = cases["100x72"]
    pts = sr.contention_cases(c)[name]
    with planner.tuning(scan_merge=MERGE_FORMS[form]):
        assert_fuse_equal(gpu_fuse(states(c), c, points=pts), sr.run(c, points=pts), f"{name}, {form}")


# ---- 4. roi ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.roi_cases(100, 72)))
def test_roi(planner, cases, states, name):
    c = cases["100x72"]
    roi, pts = sr.roi_cases(c["rows"], c["cols"])[name], sr.roi_points(c)
    assert_fuse_equal(gpu_fuse(states(c), c, points=pts, roi=roi), sr.run(c, points=pts, roi=roi), name)


def test_two_fuses_in_a_row_with_different_rois(planner, cases, states):
    """Scratch the first call left behind would show in the second: the local cell indices of the two rois differ."""
    import torch

    c = cases["100x72"]
    s = states(c)
    s.set_layers(c["elev"], c["var"])
    sp = to_struct(c["params"])
    re, rv = c["elev"], c["var"]
    for k, roi in enumerate(sr.TWO_ROIS):
        pts = c["points"] if k == 0 else sr.shuffled(c, 9)
        d_pts, d_info = device(pts), torch.full((16,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s.fuse_device(make_scan(c["T"], len(pts), roi), d_pts.data_ptr(), sp, d_info.data_ptr())
        torch.cuda.synchronize()
        re, rv, rinfo = sr.run(c, points=pts, roi=roi, elev=re, var=rv)[:3]
        e, v = s.read_layers()
        assert_fuse_equal((e, v, d_info.cpu().numpy()), (re, rv, rinfo), f"fuse {k}")


# ---- 5. arithmetic -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(MERGE_FORMS))
def test_permuted_points_give_identical_bytes(planner, cases, states, form):
    """GPU against GPU, far from the origin (the yawed and pitched case against the reference: test 1)."""
    c = cases["far,pitched"]
    with planner.tuning(scan_merge=MERGE_FORMS[form]):
        a = gpu_fuse(states(c), c)
        for seed in (3, 4):
            b = gpu_fuse(states(c), c, points=sr.shuffled(c, seed))
            assert_fuse_equal(b, a, f"permutation {seed}, {form}")


# ---- 6. move -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.MAPS))
def test_move(planner, name):
    rows, cols = sr.MAPS[name]
    e0, v0 = sr.prior_layers(rows, cols, (0.0, 0.0), (0.0, 0.0), 5)
    s = planner.scan_state(rows, cols, sr.RES, (0.0, 0.0))
    try:
        for shift in er.shifts(rows, cols) + [(-rows, -cols), (1, -1)]:
            s.set_layers(e0, v0)
            pos = er.moved_position((0.0, 0.0), shift, sr.RES)
            s.move(shift, pos)
            e, v = s.read_layers()
            assert np.array_equal(sr.bits(e), sr.bits(sr.move(e0, shift))) and np.array_equal(sr.bits(v), sr.bits(sr.move(v0, shift))), shift
            assert s.geometry()["position"] == pos
        # two moves in a row: the buffers swap back and forth
        s.set_layers(e0, v0)
        s.move((3, -2), (0.1, 0.2))
        s.move((-1, 4), (0.3, 0.4))
        e, v = s.read_layers()
        assert np.array_equal(sr.bits(e), sr.bits(sr.move(sr.move(e0, (3, -2)), (-1, 4))))
        assert np.array_equal(sr.bits(v), sr.bits(sr.move(sr.move(v0, (3, -2)), (-1, 4))))
    finally:
        s.close()


# ---- 7, 8. into the planner's snapshot ---------------------------------------------------------------------------------------------
INGESTS = [((0, 0), (10, 5, 80, 60)), ((5, 3), (0, 0, 100, 72)), ((-7, 0), (30, 14, 41, 37))]  # (shift, roi); the first neither moves nor shifts


def ingest_scan(k, pos):
    c = sr.main_case("100x72", pos=pos, seed=100 + k, width=128, height=96)
    return c, c["points"]


def test_install_and_three_ingests_equal_the_public_steps_by_hand(planner):
    """A: install, then ingest_device three times.  B: a second engine that never sees a scan state: uploaded with A's layers behind the
    install, then update_elevation with the state's roi as a host patch.  C: a third engine and state through the HOST forms."""
    import torch

    rows, cols, res = 100, 72, sr.RES
    pos = (0.0, 0.0)
    first = sr.main_case("100x72", pos=pos, seed=99)
    a, b, c = planner, FootholdPlanner(0), FootholdPlanner(0)
    sa, sc = a.scan_state(rows, cols, res, pos), c.scan_state(rows, cols, res, pos)
    try:
        for s in (sa, sc):
            s.set_layers(first["elev"], first["var"])
            s.install()
        re, rv = first["elev"], first["var"]
        ta, ea = a.read_map_layers()
        assert np.array_equal(sr.bits(ea), sr.bits(re)) and a.map_info() == {"rows": rows, "cols": cols, "resolution": res, "position": pos}
        tc, ec = c.read_map_layers()
        assert np.array_equal(sr.bits(ta), sr.bits(tc)) and np.array_equal(sr.bits(ea), sr.bits(ec))
        b.gridmapCallback(ta, ea, res, position=pos)
        for k, (shift, roi) in enumerate(INGESTS):
            pos = er.moved_position(pos, shift, res) if shift != (0, 0) else pos
            case, pts = ingest_scan(k, pos)
            scan, sp = make_scan(case["T"], len(pts), roi), to_struct(case["params"])
            d_pts, d_info = device(pts), torch.full((16,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ui_a = sa.ingest_device(scan, d_pts.data_ptr(), shift, pos, sp, d_info_ptr=d_info.data_ptr())
            torch.cuda.synchronize()
            re, rv, rinfo = sr.fuse(sr.move(re, shift), sr.move(rv, shift), res, pos, case["params"], case["T"], pts, roi)[:3]
            se, sv = sa.read_layers()
            assert_fuse_equal((se, sv, d_info.cpu().numpy()), (re, rv, rinfo), f"ingest {k}: the state")
            assert rinfo[7] > 0 and sa.geometry()["position"] == pos
            ta, ea = a.read_map_layers()
            assert np.array_equal(sr.bits(ea), sr.bits(se)), f"ingest {k}: the snapshot's elevation is not the state's"
            # B, by hand: the state's roi read back, one host patch
            r0, c0, nr, nc = roi
            ui_b = b.update_elevation(shift, pos, [(r0, c0, se[r0:r0 + nr, c0:c0 + nc])])
            tb, eb = b.read_map_layers()
            assert ui_a == ui_b and a.map_info() == b.map_info(), f"ingest {k}"
            assert np.array_equal(sr.bits(ea), sr.bits(eb)) and np.array_equal(sr.bits(ta), sr.bits(tb)), f"ingest {k}: A and B differ"
            # C: the host forms
            info_c, ui_c = sc.ingest(scan, pts, shift, pos, sp)
            tc, ec = c.read_map_layers()
            assert ui_c == ui_a and np.frombuffer(info_c.tobytes(), np.int32).tolist() == rinfo.tolist()
            assert np.array_equal(sr.bits(ec), sr.bits(ea)) and np.array_equal(sr.bits(tc), sr.bits(ta)), f"ingest {k}: host and device forms differ"
            he, hv = sc.read_layers()
            assert np.array_equal(sr.bits(he), sr.bits(se)) and np.array_equal(sr.bits(hv), sr.bits(sv))
    finally:
        sa.close()
        sc.close()
        b.close()
        c.close()


def test_host_forms_equal_device_forms(planner, cases, states):
    import torch

    c = cases["48x40"]
    s = states(c)
    dev_form, host_form = gpu_fuse(s, c), gpu_fuse(s, c, host=True)
    assert_fuse_equal(host_form, dev_form, "fuse, host against device")
    # set_layers / read_layers: the device forms, with NaN in either source
    e_src, v_src = c["elev"].copy(), c["var"].copy()
    v_src[5, 7] = np.nan
    e_src[40, 1] = -np.nan
    d_e, d_v = device(e_src), device(v_src)
    o_e, o_v = torch.zeros_like(d_e), torch.zeros_like(d_v)
    torch.cuda.synchronize()
    s.set_layers_device(d_e.data_ptr(), d_v.data_ptr())
    s.read_layers_device(o_e.data_ptr(), o_v.data_ptr())
    torch.cuda.synchronize()
    we, wv = sr.set_layers(e_src, v_src)
    assert np.array_equal(sr.bits(o_e.cpu().numpy()), sr.bits(we)) and np.array_equal(sr.bits(o_v.cpu().numpy()), sr.bits(wv))
    he, hv = s.read_layers()
    assert np.array_equal(sr.bits(he), sr.bits(we)) and np.array_equal(sr.bits(hv), sr.bits(wv))
    assert sr.bits(we)[5, 7] == sr.CLEARED and sr.bits(wv)[40, 1] == sr.CLEARED
    only_v = s.read_layers(elevation=False)
    assert only_v[0] is None and np.array_equal(sr.bits(only_v[1]), sr.bits(wv))


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_and_the_snapshot_unchanged(planner, cases):
    import torch

    c = cases["48x40"]
    rows, cols, res, pos = c["rows"], c["cols"], c["res"], c["pos"]
    L = planner._lib
    other = FootholdPlanner(0)
    s = planner.scan_state(rows, cols, res, pos)
    try:
        s.set_layers(c["elev"], c["var"])
        s.install()
        e0, v0 = s.read_layers()
        t0, m0 = planner.read_map_layers()
        d_pts = device(c["points"])
        torch.cuda.synchronize()
        good, sp = make_scan(c["T"], len(c["points"]), c["roi"]), to_struct(c["params"])

        def unchanged(what):
            torch.cuda.synchronize()
            e, v = s.read_layers()
            t, m = planner.read_map_layers()
            assert np.array_equal(sr.bits(e), sr.bits(e0)) and np.array_equal(sr.bits(v), sr.bits(v0)), what
            assert np.array_equal(sr.bits(t), sr.bits(t0)) and np.array_equal(sr.bits(m), sr.bits(m0)), what
            assert s.geometry()["position"] == pos and planner.map_info()["position"] == pos, what

        def refused(call, code, what):
            with pytest.raises(FpeError) as ei:
                call()
            assert ei.value.code == code, what
            unchanged(what)

        bad_scans = {"stride 2": make_scan(c["T"], 10, c["roi"], point_stride=2), "n_points -1": make_scan(c["T"], -1, c["roi"]),
                     "empty roi": make_scan(c["T"], 10, (0, 0, 0, 5)), "roi outside": make_scan(c["T"], 10, (40, 0, 9, 5)),
                     "non-finite transform": make_scan(np.where(np.arange(12) == 3, np.nan, c["T"]), 10, c["roi"])}
        res1 = make_scan(c["T"], 10, c["roi"])
        res1.reserved[1] = 1
        bad_scans["reserved"] = res1
        for what, scan in bad_scans.items():
            refused(lambda: s.fuse_device(scan, d_pts.data_ptr(), sp), _capi.FPE_E_INVALID_ARG, what)
            refused(lambda: s.fuse(scan, c["points"], sp), _capi.FPE_E_INVALID_ARG, what + ", host")
            refused(lambda: s.ingest_device(scan, d_pts.data_ptr(), (1, 1), (0.5, 0.5), sp), _capi.FPE_E_INVALID_ARG, what + ", ingest")
        for what, kw in {"gate 0": dict(gate=0.0), "min_z above max_z": dict(min_z=1.0, max_z=0.0), "NaN band": dict(band=np.nan),
                         "negative var_outlier": dict(var_outlier=-1.0), "var_min above var_max": dict(var_min=2.0, var_max=1.0),
                         "max_z beyond 16384": dict(max_z=20000.0), "min_range above max_range": dict(min_range=5.0, max_range=1.0)}.items():
            bad = scan_params(**kw)
            refused(lambda: s.fuse_device(good, d_pts.data_ptr(), bad), _capi.FPE_E_INVALID_ARG, what)
            refused(lambda: s.ingest(good, c["points"], (1, 1), (0.5, 0.5), bad), _capi.FPE_E_INVALID_ARG, what + ", ingest")
        # null arguments, straight through ctypes
        null = [L.fpe_scan_fuse_device(s._s, None, C.byref(good), C.c_void_p(d_pts.data_ptr()), None, None),
                L.fpe_scan_fuse_device(s._s, C.byref(sp), None, C.c_void_p(d_pts.data_ptr()), None, None),
                L.fpe_scan_fuse_device(s._s, C.byref(sp), C.byref(good), None, None, None),
                L.fpe_scan_fuse_device(None, C.byref(sp), C.byref(good), C.c_void_p(d_pts.data_ptr()), None, None),
                L.fpe_scan_fuse(s._s, C.byref(sp), C.byref(good), None, None),
                L.fpe_scan_read_layers(s._s, None, None), L.fpe_scan_set_layers(s._s, None, None), L.fpe_scan_move(s._s, None, None, None),
                L.fpe_scan_install(None, s._s, None, None), L.fpe_scan_geometry(s._s, None)]
        assert null == [_capi.FPE_E_INVALID_ARG] * len(null)
        unchanged("null arguments")
        refused(lambda: s.move((1, 0), (np.nan, 0.0)), _capi.FPE_E_INVALID_ARG, "move to a NaN position")
        refused(lambda: s.ingest_device(good, d_pts.data_ptr(), (1, 0), (np.inf, 0.0), sp), _capi.FPE_E_INVALID_ARG, "ingest at an infinite position")
        refused(lambda: s.ingest_device(good, d_pts.data_ptr(), (0, 0), pos, sp, filter_params=planner.filter_params(normal_radius=-1.0)),
                _capi.FPE_E_INVALID_ARG, "ingest with a bad filter radius")
        # the snapshot must be of the state's size and resolution; and there must be one
        with pytest.raises(FpeError) as ei:
            other_state = other.scan_state(rows, cols, res, pos)
            try:
                other_state.ingest_device(good, d_pts.data_ptr(), (0, 0), pos, sp)
            finally:
                other_state.close()
        assert ei.value.code == _capi.FPE_E_NO_MAP
        planner.gridmapCallback(np.ones((rows + 1, cols), np.float32), np.zeros((rows + 1, cols), np.float32), res, position=pos)
        with pytest.raises(FpeError) as ei:
            s.ingest_device(good, d_pts.data_ptr(), (0, 0), pos, sp)
        assert ei.value.code == _capi.FPE_E_INVALID_ARG
        planner.gridmapCallback(np.ones((rows, cols), np.float32), np.zeros((rows, cols), np.float32), 0.03, position=pos)
        with pytest.raises(FpeError) as ei:
            s.ingest(good, c["points"], (0, 0), pos, sp)
        assert ei.value.code == _capi.FPE_E_INVALID_ARG
        e, v = s.read_layers()
        assert np.array_equal(sr.bits(e), sr.bits(e0)) and np.array_equal(sr.bits(v), sr.bits(v0)) and s.geometry()["position"] == pos
        # a state belongs to its engine; the tuning key takes 0, 1, 2
        assert L.fpe_scan_install(other._h, s._s, None, None) == _capi.FPE_E_INVALID_ARG
        with pytest.raises(FpeError):
            planner.set_tuning(scan_merge=3)
        planner.set_tuning(scan_merge=0)
    finally:
        s.close()
        other.close()
