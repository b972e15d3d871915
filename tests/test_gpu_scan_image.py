"""Scan images on the device (fpe_scan_*_image*; include/fpe.h, point 6 of the scan block) against the numpy statement of the contract
(tests/scan_image_reference.py: the pixel rule, then the existing references of the fuse, the clear and the close on its points).  Every
comparison is of bits: both layers over the whole state, every word of every info record, and — for the way into the planner's
snapshot — both snapshot layers against a second engine that is driven through the POINT entry points with the reference's points.

That the cases show every drop class, every cell class, a cell with more than 64 kept points, runs across row ends and every counter
of the clear is asserted of the reference alone in tests/test_cpu_scan_image.py.  Shapes: maps of 100 x 72 and 48 x 40 at 2 cm, images
of at most 160 x 120 pixels."""
import ctypes as C

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import (FootholdPlanner, FpeError, make_scan, make_scan_image, scan_clear_params, scan_close_params,
                                                      scan_params)
from tests import elevation_update_reference as er
from tests import scan_clear_reference as cr
from tests import scan_close_reference as kr
from tests import scan_image_reference as ir
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
    return ir.all_cases()


@pytest.fixture(scope="module")
def states(planner):
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
    """A reference result computed once per key and shared by the forms."""
    memo = {}

    def get(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]

    return get


def sp_struct(p):
    return scan_params(**{k: (int(v) if k == "replace_count" else float(v)) for k, v in p.items()})


def cp_struct(cp):
    return scan_clear_params(**{k: (float(v) if k in cr.FLOAT_FIELDS else int(v)) for k, v in cp.items()})


def kp_struct(kp):
    return scan_close_params(**{k: (float(v) if k == "max_spread" else int(v)) for k, v in kp.items()})


def device(a):
    """Any array on the device as its bytes (uint16 images included); the tensor keeps the memory alive."""
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)).cuda()


def fresh_info():
    import torch

    return torch.full((16,), -7, dtype=torch.int32, device="cuda")


class DeviceImage:
    """A case's image and tables on the device, and the descriptor that names them (offset: the first element, for crops)."""

    def __init__(self, im, image, offset=0):
        self.d_image = device(image)
        self.tables = [device(im[k]) if im[k] is not None else None for k in ("row_dir", "col_dir")]
        kw = dict(im, row_dir=self.tables[0].data_ptr() if self.tables[0] is not None else None,
                  col_dir=self.tables[1].data_ptr() if self.tables[1] is not None else None)
        self.im = make_scan_image(**kw)
        self.ptr = self.d_image.data_ptr() + offset * np.asarray(image).dtype.itemsize


def scan_of(case, roi=None):
    return make_scan(case["T"], len(case["points"]), case["roi"] if roi is None else roi)


def gpu_fuse_image(state, case, roi=None, elev=None, var=None, host=False, set_layers=True):
    """set_layers, one image fuse (device form unless `host`) -> (elevation, variance, the info's sixteen words)."""
    import torch

    if set_layers:
        state.set_layers(case["elev"] if elev is None else elev, case["var"] if var is None else var)
    scan, sp = scan_of(case, roi), sp_struct(case["params"])
    if host:
        words = np.frombuffer(state.fuse_image(scan, make_scan_image(**case["im"]), case["image"], sp).tobytes(), np.int32)
    else:
        di, d_info = DeviceImage(case["im"], case["image"]), fresh_info()
        torch.cuda.synchronize()
        state.fuse_image_device(scan, di.im, di.ptr, sp, d_info.data_ptr())
        torch.cuda.synchronize()
        words = d_info.cpu().numpy()
    return (*state.read_layers(), words)


def gpu_clear_image(state, case, cp=None, roi=None, elev=None, var=None, host=False, set_layers=True):
    import torch

    if set_layers:
        state.set_layers(case["elev"] if elev is None else elev, case["var"] if var is None else var)
    scan, sp, cps = scan_of(case, roi), sp_struct(case["params"]), cp_struct(cr.params() if cp is None else cp)
    if host:
        words = cr.words(state.clear_image(scan, make_scan_image(**case["im"]), case["image"], sp, cps))
    else:
        di, d_info = DeviceImage(case["im"], case["image"]), fresh_info()
        torch.cuda.synchronize()
        state.clear_image_device(scan, di.im, di.ptr, sp, cps, d_info.data_ptr())
        torch.cuda.synchronize()
        words = d_info.cpu().numpy()
    return (*state.read_layers(), words)


def gpu_fuse_points(state, case, points=None, roi=None):
    """One device fuse of POINTS into the state as it is."""
    import torch

    points = case["points"] if points is None else points
    d_pts, d_info = device(points), fresh_info()
    torch.cuda.synchronize()
    state.fuse_device(make_scan(case["T"], len(points), case["roi"] if roi is None else roi), d_pts.data_ptr(), sp_struct(case["params"]), d_info.data_ptr())
    torch.cuda.synchronize()
    return (*state.read_layers(), d_info.cpu().numpy())


def gpu_clear_points(state, case, cp=None, points=None):
    import torch

    points = case["points"] if points is None else points
    d_pts, d_info = device(points), fresh_info()
    torch.cuda.synchronize()
    state.clear_device(make_scan(case["T"], len(points), case["roi"]), d_pts.data_ptr(), sp_struct(case["params"]),
                       cp_struct(cr.params() if cp is None else cp), d_info.data_ptr())
    torch.cuda.synchronize()
    return (*state.read_layers(), d_info.cpu().numpy())


def words_of(info):
    return info if isinstance(info, np.ndarray) and info.dtype == np.int32 else np.frombuffer(np.asarray(info).tobytes(), np.int32)


def assert_equal(got, want, what):
    """got: (e, v, sixteen words); want: the same, or a reference's (e, v, info, ...)."""
    (e, v, words), (re, rv, rinfo) = got, want[:3]
    rwords = words_of(rinfo)
    print(what, "info", words.tolist())
    assert words.tolist() == rwords.tolist(), f"{what}: info {words.tolist()} against {rwords.tolist()}"
    de, dv = sr.bits(e) != sr.bits(re), sr.bits(v) != sr.bits(rv)
    assert not de.any(), f"{what}: {int(de.sum())} elevation cells differ, first at {np.argwhere(de)[0].tolist()}"
    assert not dv.any(), f"{what}: {int(dv.sum())} variance cells differ, first at {np.argwhere(dv)[0].tolist()}"


# ---- 1. the fuse -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ir.all_cases()))
def test_fuse_image_equals_the_reference_on_every_byte(cases, states, name):
    c = cases[name]
    assert_equal(gpu_fuse_image(states(c), c), ir.fuse(c), name)


@pytest.mark.parametrize("roi", list(sr.roi_cases(100, 72)))
@pytest.mark.parametrize("name", ["depth_u16,100x72", "lidar_f32,100x72", "one cell"])
def test_fuse_image_rois(cases, states, name, roi):
    c = cases[name]
    r = sr.roi_cases(c["rows"], c["cols"])[roi]
    assert_equal(gpu_fuse_image(states(c), c, roi=r), ir.fuse(c, roi=r), f"{name}, {roi}")


def test_two_image_fuses_in_a_row_with_different_rois(cases, states):
    """Scratch the first call left behind would show in the second: the local cell indices of the two rois differ."""
    a, b = cases["depth_u16,100x72"], cases["depth_f32"]
    s = states(a)
    re, rv = a["elev"], a["var"]
    for k, (c, roi) in enumerate(zip((a, b), sr.TWO_ROIS)):
        want = ir.fuse(c, roi=roi, elev=re, var=rv)
        assert_equal(gpu_fuse_image(s, c, roi=roi, elev=re, var=rv, set_layers=k == 0), want, f"fuse {k}")
        re, rv = want[:2]


def test_a_crop_is_a_pointer_offset_and_a_pitch(cases, states):
    """The window [1:, 1:] of the pitched image: an odd element offset (a 2-byte aligned address) and the parent's pitch."""
    import torch

    c = cases["depth_u16,pitch+7"]
    im = dict(c["im"], width=c["im"]["width"] - 1, height=c["im"]["height"] - 1)
    offset = c["im"]["row_pitch"] + 1
    crop = dict(c, im=im, points=ir.points(im, c["image"].reshape(-1)[offset:]))
    s = states(c)
    s.set_layers(c["elev"], c["var"])
    di, d_info = DeviceImage(im, c["image"], offset), fresh_info()
    torch.cuda.synchronize()
    s.fuse_image_device(scan_of(crop), di.im, di.ptr, sp_struct(c["params"]), d_info.data_ptr())
    torch.cuda.synchronize()
    assert_equal((*s.read_layers(), d_info.cpu().numpy()), ir.fuse(crop), "crop")


# ---- 2. the clear, in every form of the ray pass -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(ir.main_cases()))
def test_clear_image_equals_the_reference_on_every_byte(planner, cases, states, reference, name, form):
    c = cases[name]
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear_image(states(c), c), reference(name, lambda: ir.clear(c)), f"{name}, {form}")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["depth_u16,100x72", "depth_u16,48x40"])
def test_clear_image_ghost_state(planner, cases, states, reference, name, form):
    """The ghost goes, nothing beside it."""
    c = cases[name]
    ge, gv = cr.ghost_state(c)
    want = reference("ghost " + name, lambda: ir.clear(c, elev=ge, var=gv))
    assert 1 <= want[2]["cells_cleared"] <= 36
    with planner.tuning(**FORMS[form]):
        got = gpu_clear_image(states(c), c, elev=ge, var=gv)
    assert_equal(got, want, f"ghost, {name}, {form}")
    r0, c0, nr, nc = cr.ghost_box(c)
    outside = np.ones(ge.shape, bool)
    outside[r0:r0 + nr, c0:c0 + nc] = False
    assert np.array_equal(sr.bits(got[0])[outside], sr.bits(ge)[outside])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["depth_u16,100x72", "far,pitched", "lidar_f32,100x72"])
def test_clear_image_every_per_point_counter(planner, cases, states, reference, name, form):
    c = cases[name]
    cp = cr.params(**cr.EVERY_COUNTER)
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear_image(states(c), c, cp=cp), reference("every counter " + name, lambda: ir.clear(c, cp=cp)), f"every counter, {name}, {form}")


@pytest.mark.parametrize("ray_stride", [1, 2, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_clear_image_launch_edges_and_ray_strides(planner, cases, states, reference, form, ray_stride):
    """The small images around a wavefront and a workgroup, the stepped and pitched image and the contention images; min_hits 1, so that
    the few rays of the small ones clear cells."""
    cp = cr.params(min_hits=1, ray_stride=ray_stride)
    cleared = 0
    with planner.tuning(**FORMS[form]):
        for name in list(ir.edge_cases()) + ["depth_f32,steps(2,3),pitch+7", "one row"]:
            c = cases[name]
            want = reference(f"edges {name} {ray_stride}", lambda: ir.clear(c, cp=cp))
            cleared += int(want[2]["cells_cleared"])
            assert_equal(gpu_clear_image(states(c), c, cp=cp), want, f"{name}, ray_stride {ray_stride}, {form}")
    assert cleared > 0


@pytest.mark.parametrize("form", list(FORMS))
def test_clear_image_contention(planner, cases, states, reference, form):
    """4 096 rays through the same few cells under the sensor, over a prior that stands above the sensor."""
    c = cases["one cell"]
    e, v = cr.raised(c)
    cp = cr.params(**cr.CONTENTION)
    with planner.tuning(**FORMS[form]):
        assert_equal(gpu_clear_image(states(c), c, cp=cp, elev=e, var=v), reference("contention", lambda: ir.clear(c, cp=cp, elev=e, var=v)), f"one cell, {form}")


# ---- 3. the scratch at rest, image and point forms mixed ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TWO_FORMS)
def test_image_and_point_forms_share_the_scratch(planner, cases, states, form):
    c, other = cases["depth_u16,100x72"], cases["depth_f32"]
    s = states(c)
    with planner.tuning(**FORMS[form]):
        # clear_image -> fuse (points)
        r_clear = ir.clear(c)
        assert r_clear[2]["cells_hit"] > r_clear[2]["cells_cleared"] > 0  # cells with hits below min_hits: their hits must be gone too
        assert_equal(gpu_clear_image(s, c), r_clear, f"clear_image, {form}")
        r_fuse = sr.run(c, elev=r_clear[0], var=r_clear[1])
        assert_equal(gpu_fuse_points(s, c), r_fuse, f"fuse after clear_image, {form}")
        # fuse_image -> clear (points) -> fuse_image, on from there, with the other image
        r1 = ir.fuse(other, elev=r_fuse[0], var=r_fuse[1])
        assert_equal(gpu_fuse_image(s, other, set_layers=False), r1, f"fuse_image, {form}")
        r2 = cr.run(c, elev=r1[0], var=r1[1])
        assert_equal(gpu_clear_points(s, c), r2, f"clear after fuse_image, {form}")
        r3 = ir.fuse(other, elev=r2[0], var=r2[1])
        assert_equal(gpu_fuse_image(s, other, set_layers=False), r3, f"second fuse_image, {form}")


# ---- 4. image form against point form, GPU against GPU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ir.main_cases()) + ["one cell", "2x65,pitch70"])
def test_image_forms_leave_the_bytes_of_the_point_forms(cases, states, name):
    """fuse_device / clear_device on points(image) uploaded as floats, against the image forms."""
    c = cases[name]
    s = states(c)
    s.set_layers(c["elev"], c["var"])
    by_points = gpu_fuse_points(s, c)
    assert_equal(gpu_fuse_image(s, c), by_points, f"{name}: fuse")
    s.set_layers(c["elev"], c["var"])
    by_points = gpu_clear_points(s, c)
    assert_equal(gpu_clear_image(s, c), by_points, f"{name}: clear")


# ---- 5. into the planner's snapshot ------------------------------------------------------------------------------------------------------
# (shift, roi, the image): every sign of the shift on both axes; the first neither moves nor shifts
INGESTS = [((0, 0), (10, 5, 80, 60), "depth_u16"), ((5, -3), (0, 0, 100, 72), "lidar_f32"), ((-7, 2), (30, 14, 41, 37), "depth_f32")]
MODES = {"ingest": (False, False), "ingest_clear": (True, False), "ingest_closed": (True, True)}


@pytest.mark.parametrize("mode", list(MODES))
def test_install_and_three_ingest_images_equal_the_point_entry_points(planner, mode):
    """A: install, then ingest_image_device three times.  B: a second engine and state through the POINT entry points with the
    reference's points.  C: a third through the HOST image form.  The state is also compared with the reference's move, clear and fuse,
    and with close parameters the snapshot with close(whole state) of the reference."""
    import torch

    with_clear, with_close = MODES[mode]
    rows, cols, res = 100, 72, sr.RES
    pos = (0.0, 0.0)
    first = sr.main_case("100x72", pos=pos, seed=99)
    cp, kp = cr.params(), kr.params()
    cps, kps = (cp_struct(cp) if with_clear else None), (kp_struct(kp) if with_close else None)
    a, b, c = planner, FootholdPlanner(0), FootholdPlanner(0)
    sa, sb, sc = (p.scan_state(rows, cols, res, pos) for p in (a, b, c))
    try:
        for s in (sa, sb, sc):
            s.set_layers(first["elev"], first["var"])
            s.install_closed(kps) if with_close else s.install()
        re, rv = first["elev"], first["var"]
        for k, (shift, roi, kind) in enumerate(INGESTS):
            pos = er.moved_position(pos, shift, res) if shift != (0, 0) else pos
            case = getattr(ir, kind)("100x72", pos=pos, seed=100 + k)
            pts, sp = case["points"], sp_struct(case["params"])
            scan = make_scan(case["T"], len(pts), roi)
            di, d_pts = DeviceImage(case["im"], case["image"]), device(pts)
            ia, ib = [fresh_info() for _ in range(3)], [fresh_info() for _ in range(3)]
            torch.cuda.synchronize()
            ui_a = sa.ingest_image_device(scan, di.im, di.ptr, shift, pos, sp, cps, kps, d_clear_info_ptr=ia[0].data_ptr(), d_info_ptr=ia[1].data_ptr(),
                                          d_close_info_ptr=ia[2].data_ptr())
            if with_close:
                ui_b = sb.ingest_closed_device(scan, d_pts.data_ptr(), shift, pos, sp, cps, kps, d_clear_info_ptr=ib[0].data_ptr(), d_info_ptr=ib[1].data_ptr(),
                                               d_close_info_ptr=ib[2].data_ptr())
            elif with_clear:
                ui_b = sb.ingest_clear_device(scan, d_pts.data_ptr(), shift, pos, sp, cps, d_clear_info_ptr=ib[0].data_ptr(), d_info_ptr=ib[1].data_ptr())
            else:
                ui_b = sb.ingest_device(scan, d_pts.data_ptr(), shift, pos, sp, d_info_ptr=ib[1].data_ptr())
            torch.cuda.synchronize()
            wa, wb = [t.cpu().numpy().tolist() for t in ia], [t.cpu().numpy().tolist() for t in ib]
            assert wa == wb and ui_a == ui_b and a.map_info() == b.map_info(), f"{mode} {k}: infos"
            assert wa[0] == ([-7] * 16 if not with_clear else wa[0]) and wa[2] == ([-7] * 16 if not with_close else wa[2])  # an unused info is not written
            # the reference: move, clear, fuse
            re, rv = sr.move(re, shift), sr.move(rv, shift)
            if with_clear:
                re, rv, cinfo, _ = cr.clear(re, rv, res, pos, case["params"], cp, case["T"], pts, roi)
                assert wa[0] == cr.words(cinfo).tolist(), f"{mode} {k}: the clear's info"
            re, rv, rinfo = sr.fuse(re, rv, res, pos, case["params"], case["T"], pts, roi)[:3]
            assert wa[1] == rinfo.tolist(), f"{mode} {k}: the fuse's info"
            (ea, va), (eb, vb) = sa.read_layers(), sb.read_layers()
            assert np.array_equal(sr.bits(ea), sr.bits(re)) and np.array_equal(sr.bits(va), sr.bits(rv)), f"{mode} {k}: the state against the reference"
            assert np.array_equal(sr.bits(ea), sr.bits(eb)) and np.array_equal(sr.bits(va), sr.bits(vb)), f"{mode} {k}: the states of A and B differ"
            (ta, ma), (tb, mb) = a.read_map_layers(), b.read_map_layers()
            assert np.array_equal(sr.bits(ta), sr.bits(tb)) and np.array_equal(sr.bits(ma), sr.bits(mb)), f"{mode} {k}: the snapshots of A and B differ"
            if with_close:
                assert np.array_equal(sr.bits(ma), sr.bits(kr.close(re, kp)[0])), f"{mode} {k}: the snapshot is not close(whole state)"
            else:
                assert np.array_equal(sr.bits(ma), sr.bits(ea)), f"{mode} {k}: the snapshot's elevation is not the state's"
            # C: the host form
            cinfo_c, info_c, kinfo_c, ui_c = sc.ingest_image(scan, make_scan_image(**case["im"]), case["image"], shift, pos, sp, cps, kps)
            assert ui_c == ui_a and words_of(info_c).tolist() == wa[1], f"{mode} {k}: host form"
            assert (cinfo_c is None) == (not with_clear) and (cinfo_c is None or words_of(cinfo_c).tolist() == wa[0])
            assert (kinfo_c is None) == (not with_close) and (kinfo_c is None or words_of(kinfo_c).tolist() == wa[2])
            (ec, vc), (tc, mc) = sc.read_layers(), c.read_map_layers()
            assert np.array_equal(sr.bits(ec), sr.bits(ea)) and np.array_equal(sr.bits(vc), sr.bits(va)), f"{mode} {k}: host and device states differ"
            assert np.array_equal(sr.bits(tc), sr.bits(ta)) and np.array_equal(sr.bits(mc), sr.bits(ma)), f"{mode} {k}: host and device snapshots differ"
    finally:
        for s in (sa, sb, sc):
            s.close()
        b.close()
        c.close()


def test_ingest_image_with_close_parameters_alone(planner, cases):
    """kp given, cp NULL: fpe_scan_ingest_closed without the clear."""
    import torch

    c = cases["depth_u16,100x72"]
    kp = kr.params()
    b = FootholdPlanner(0)
    sa, sb = (p.scan_state(c["rows"], c["cols"], c["res"], c["pos"]) for p in (planner, b))
    try:
        for s in (sa, sb):
            s.set_layers(c["elev"], c["var"])
            s.install_closed(kp_struct(kp))
        di, d_pts = DeviceImage(c["im"], c["image"]), device(c["points"])
        torch.cuda.synchronize()
        ui_a = sa.ingest_image_device(scan_of(c), di.im, di.ptr, (0, 0), c["pos"], sp_struct(c["params"]), None, kp_struct(kp))
        ui_b = sb.ingest_closed_device(scan_of(c), d_pts.data_ptr(), (0, 0), c["pos"], sp_struct(c["params"]), None, kp_struct(kp))
        torch.cuda.synchronize()
        want = ir.fuse(c)
        assert ui_a == ui_b
        assert_equal((*sa.read_layers(), want[2]), want, "the state")
        (ta, ma), (tb, mb) = planner.read_map_layers(), b.read_map_layers()
        assert np.array_equal(sr.bits(ma), sr.bits(kr.close(want[0], kp)[0])) and np.array_equal(sr.bits(ma), sr.bits(mb)) and np.array_equal(sr.bits(ta), sr.bits(tb))
    finally:
        sa.close()
        sb.close()
        b.close()


# ---- 6. host forms against device forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth_u16,pitch+7", "depth_f32,steps(2,3),pitch+7", "lidar_f32,100x72", "one cell", "1x1", "2x65,pitch70"])
def test_host_forms_equal_device_forms(planner, cases, states, name):
    """The host forms stage the image at its own size and the two tables: a pitched uint16 image, a pitched float image, a spherical
    one, and the smallest."""
    c = cases[name]
    s = states(c)
    assert_equal(gpu_fuse_image(s, c, host=True), gpu_fuse_image(s, c), f"{name}: fuse, host against device")
    assert_equal(gpu_clear_image(s, c, host=True), gpu_clear_image(s, c), f"{name}: clear, host against device")
    # a null info is allowed in both forms
    s.set_layers(c["elev"], c["var"])
    scan, sp, im = scan_of(c), sp_struct(c["params"]), make_scan_image(**c["im"])
    assert planner._lib.fpe_scan_fuse_image(s._s, C.byref(sp), C.byref(scan), C.byref(im), c["image"].ctypes.data_as(C.c_void_p), None) == _capi.FPE_OK
    want = ir.fuse(c)
    assert_equal((*s.read_layers(), want[2]), want, f"{name}: after a call without an info")


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_the_snapshot_and_the_outputs_unchanged(planner, cases):
    import torch

    c = cases["depth_u16,48x40"]
    lid = cases["lidar_f32,48x40"]
    rows, cols, res, pos = c["rows"], c["cols"], c["res"], c["pos"]
    L = planner._lib
    s = planner.scan_state(rows, cols, res, pos)
    try:
        s.set_layers(c["elev"], c["var"])
        s.install()
        e0, v0 = s.read_layers()
        t0, m0 = planner.read_map_layers()
        di, dl = DeviceImage(c["im"], c["image"]), DeviceImage(lid["im"], lid["image"])
        infos = [fresh_info() for _ in range(3)]
        torch.cuda.synchronize()
        good, sp, cp, kp = scan_of(c), sp_struct(c["params"]), scan_clear_params(), scan_close_params()
        ptrs = dict(d_clear_info_ptr=infos[0].data_ptr(), d_info_ptr=infos[1].data_ptr(), d_close_info_ptr=infos[2].data_ptr())

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
            assert all(t.cpu().numpy().tolist() == [-7] * 16 for t in infos), what

        def every_form(scan, im, ptr, what, sp=sp, cp=cp, host_image=None):
            refused(lambda: s.fuse_image_device(scan, im, ptr, sp, infos[1].data_ptr()), what + ", fuse")
            refused(lambda: s.clear_image_device(scan, im, ptr, sp, cp, infos[0].data_ptr()), what + ", clear")
            refused(lambda: s.ingest_image_device(scan, im, ptr, (1, 1), (0.5, 0.5), sp, None, None, **ptrs), what + ", ingest")
            refused(lambda: s.ingest_image_device(scan, im, ptr, (1, 1), (0.5, 0.5), sp, cp, kp, **ptrs), what + ", ingest with cp and kp")
            if host_image is not None:
                refused(lambda: s.fuse_image(scan, im, host_image, sp), what + ", host fuse")
                refused(lambda: s.clear_image(scan, im, host_image, sp, cp), what + ", host clear")
                refused(lambda: s.ingest_image(scan, im, host_image, (1, 1), (0.5, 0.5), sp, cp, kp), what + ", host ingest")

        big = np.zeros(4097 * 160, np.uint16)  # enough elements for the binding's own size check of the widest refused descriptor
        for what, kw in ir.REFUSED.items():
            every_form(good, make_scan_image(**dict(c["im"], **kw)), di.ptr, what, host_image=big if what != "more than FPE_SCAN_MAX_POINTS" else None)
        for k in (0, 1):
            im = make_scan_image(**c["im"])
            im.reserved[k] = 5
            every_form(good, im, di.ptr, f"reserved[{k}]", host_image=c["image"])
        for k, name in enumerate(("row_dir", "col_dir")):
            im = make_scan_image(**{**lid["im"], "row_dir": dl.tables[0].data_ptr(), "col_dir": dl.tables[1].data_ptr(), name: None})
            every_form(scan_of(lid), im, dl.ptr, f"spherical without {name}")
        for n in (len(c["points"]) - 1, len(c["points"]) + 1, 0):
            every_form(make_scan(c["T"], n, c["roi"]), di.im, di.ptr, f"n_points {n}", host_image=c["image"])
        # everything the point form refuses
        n = len(c["points"])
        bad_scans = {"stride 2": make_scan(c["T"], n, c["roi"], point_stride=2), "empty roi": make_scan(c["T"], n, (0, 0, 0, 5)),
                     "roi outside": make_scan(c["T"], n, (40, 0, 9, 5)), "non-finite transform": make_scan(np.where(np.arange(12) == 3, np.nan, c["T"]), n, c["roi"])}
        for what, scan in bad_scans.items():
            every_form(scan, di.im, di.ptr, what, host_image=c["image"])
        for what, kw in {"gate 0": dict(gate=0.0), "min_z above max_z": dict(min_z=1.0, max_z=0.0), "NaN band": dict(band=np.nan)}.items():
            every_form(good, di.im, di.ptr, what, sp=scan_params(**kw))
        for what, kw in {"sample_step 0": dict(sample_step=0.0), "min_hits 0": dict(min_hits=0), "reserved": dict(reserved=7)}.items():
            bad = scan_clear_params(**kw)
            refused(lambda: s.clear_image_device(good, di.im, di.ptr, sp, bad, infos[0].data_ptr()), what)
            refused(lambda: s.ingest_image_device(good, di.im, di.ptr, (1, 1), (0.5, 0.5), sp, bad, None, **ptrs), what + ", ingest")
            refused(lambda: s.ingest_image(good, make_scan_image(**c["im"]), c["image"], (1, 1), (0.5, 0.5), sp, bad, kp), what + ", host ingest")
        for what, kw in {"reach 0": dict(reach=0), "max_gap 99": dict(max_gap=99), "NaN spread": dict(max_spread=np.nan)}.items():
            refused(lambda: s.ingest_image_device(good, di.im, di.ptr, (1, 1), (0.5, 0.5), sp, cp, scan_close_params(**kw), **ptrs), what)
        refused(lambda: s.ingest_image_device(good, di.im, di.ptr, (1, 0), (np.inf, 0.0), sp, cp, None, **ptrs), "ingest at an infinite position")
        refused(lambda: s.ingest_image_device(good, di.im, di.ptr, (0, 0), pos, sp, cp, None, filter_params=planner.filter_params(normal_radius=-1.0), **ptrs),
                "ingest with a bad filter radius")
        # null arguments, straight through ctypes
        p = C.c_void_p(di.ptr)
        sh, ps = (C.c_int32 * 2)(0, 0), (C.c_double * 2)(*pos)
        null = [L.fpe_scan_fuse_image_device(s._s, C.byref(sp), C.byref(good), None, p, None, None),
                L.fpe_scan_fuse_image_device(s._s, C.byref(sp), C.byref(good), C.byref(di.im), None, None, None),
                L.fpe_scan_fuse_image_device(s._s, None, C.byref(good), C.byref(di.im), p, None, None),
                L.fpe_scan_fuse_image_device(s._s, C.byref(sp), None, C.byref(di.im), p, None, None),
                L.fpe_scan_fuse_image_device(None, C.byref(sp), C.byref(good), C.byref(di.im), p, None, None),
                L.fpe_scan_fuse_image(s._s, C.byref(sp), C.byref(good), C.byref(di.im), None, None),
                L.fpe_scan_clear_image_device(s._s, C.byref(sp), None, C.byref(good), C.byref(di.im), p, None, None),
                L.fpe_scan_clear_image_device(s._s, C.byref(sp), C.byref(cp), C.byref(good), None, p, None, None),
                L.fpe_scan_clear_image(s._s, C.byref(sp), C.byref(cp), C.byref(good), C.byref(di.im), None, None),
                L.fpe_scan_ingest_image_device(planner._h, s._s, None, C.byref(sp), None, None, C.byref(good), None, p, sh, ps, None, None, None, None, None),
                L.fpe_scan_ingest_image_device(planner._h, s._s, None, C.byref(sp), None, None, C.byref(good), C.byref(di.im), None, sh, ps, None, None, None, None, None),
                L.fpe_scan_ingest_image_device(planner._h, s._s, None, C.byref(sp), None, None, C.byref(good), C.byref(di.im), p, None, ps, None, None, None, None, None),
                L.fpe_scan_ingest_image_device(None, s._s, None, C.byref(sp), None, None, C.byref(good), C.byref(di.im), p, sh, ps, None, None, None, None, None)]
        assert null == [_capi.FPE_E_INVALID_ARG] * len(null)
        torch.cuda.synchronize()
        e, v = s.read_layers()
        assert np.array_equal(sr.bits(e), sr.bits(e0)) and np.array_equal(sr.bits(v), sr.bits(v0))
        # and a valid call with every info null goes through: the state changes, the snapshot follows
        assert L.fpe_scan_ingest_image_device(planner._h, s._s, None, C.byref(sp), C.byref(cp), None, C.byref(good), C.byref(di.im), p, sh, ps, None, None, None,
                                              None, None) == _capi.FPE_OK
        torch.cuda.synchronize()
        ce, cv = ir.clear(c)[:2]
        want = ir.fuse(c, elev=ce, var=cv)
        e, v = s.read_layers()
        assert np.array_equal(sr.bits(e), sr.bits(want[0])) and np.array_equal(sr.bits(v), sr.bits(want[1]))
        assert np.array_equal(sr.bits(planner.read_map_layers()[1]), sr.bits(e))
    finally:
        s.close()
