"""The scan images' contract without a GPU (fpe_scan_*_image*; include/fpe.h, point 6 of the scan block): the numpy statement
(tests/scan_image_reference.py) against a 4 x 4 image worked out by hand, the library's host statement of the rule
(fpe_scan_image_points) against it bit for bit on every case the GPU tests use, every refusal of fpe_scan_image_validate and the valid
edges, the C side of the new ABI — and, of the reference alone, that each GPU case shows what it is there to show."""
import ctypes as C

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import (FpeError, make_scan, make_scan_image, scan_clear_params, scan_image_points, scan_image_selected,
                                                      scan_image_validate, scan_params)
from tests import abi_c
from tests import scan_clear_reference as cr
from tests import scan_image_reference as ir
from tests import scan_reference as sr

F32 = np.float32
OK, BAD = _capi.FPE_OK, _capi.FPE_E_INVALID_ARG


@pytest.fixture(scope="module")
def cases():
    return ir.all_cases()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- 1. a 4 x 4 image by hand ------------------------------------------------------------------------------------------------------
# raw[v, u] = 1024 (v + 1) + 512 u at scale 2^-10: d = (v + 1) + u / 2.  Steps (2, 2) select (0, 0), (0, 2), (2, 0), (2, 2); the last is invalid.
HAND_D = np.array([[1024.0 * (v + 1) + 512.0 * u for u in range(4)] for v in range(4)])
NANS = [np.nan] * 3
HAND = {
    # fx 2, fy 4, cx 1, cy 2:  x = (u - 1) d / 2,  y = (v - 2) d / 4,  z = d
    "pinhole": (dict(fx=2.0, fy=4.0, cx=1.0, cy=2.0), [[-0.5, -0.5, 1.0], [1.0, -1.0, 2.0], [-1.5, 0.0, 3.0], NANS]),
    # rows (1, 0) and (1/2, -1/2), columns (1, 0) and (0, 1):  w = d ce,  x = w ca,  y = w sa,  z = d se
    "spherical": (dict(row_dir=[[1.0, 0.0], [9.0, 9.0], [0.5, -0.5], [9.0, 9.0]], col_dir=[[1.0, 0.0], [9.0, 9.0], [0.0, 1.0], [9.0, 9.0]]),
                  [[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [1.5, 0.0, -1.5], NANS]),
}


@pytest.mark.parametrize("fmt", ["u16", "f32"])
@pytest.mark.parametrize("model", list(HAND))
def test_a_four_by_four_image_by_hand(model, fmt):
    kw, want = HAND[model]
    img = HAND_D.astype(np.uint16 if fmt == "u16" else F32)
    img[2, 2] = 0 if fmt == "u16" else np.nan
    im = ir.descriptor(model, fmt, 4, 4, row_step=2, col_step=2, depth_scale=2.0 ** -10, **kw)
    want = np.array(want, F32)
    assert [len(a) for a in ir.selected(im)] == [2, 2] and scan_image_selected(make_scan_image(**im)) == (2, 2)
    for got in (ir.points(im, img), scan_image_points(make_scan_image(**im), img)):
        assert got.shape == (4, 3) and np.array_equal(got[:3], want[:3]) and np.isnan(got[3]).all()
        assert bits(got[3]).tolist() == [0x7FC00000] * 3
    # every pixel (steps 1): the invalid one alone is NaN, and z is d in the pinhole model
    im1 = dict(im, row_step=1, col_step=1)
    full = ir.points(im1, img)
    assert np.isnan(full).any(axis=1).tolist() == [k == 10 for k in range(16)]
    if model == "pinhole":
        assert np.array_equal(np.delete(full[:, 2], 10), np.delete(HAND_D.reshape(-1) / 1024.0, 10).astype(F32))


# ---- 2. the library's host statement against the reference, bit for bit -------------------------------------------------------------
@pytest.mark.parametrize("name", list(ir.all_cases()))
def test_image_points_equal_the_reference_bit_for_bit(cases, name):
    c = cases[name]
    got = scan_image_points(make_scan_image(**c["im"]), c["image"])
    assert got.shape == c["points"].shape == (int(np.prod([len(a) for a in ir.selected(c["im"])])), 3)
    diff = bits(got) != bits(c["points"])
    assert not diff.any(), f"{name}: {int(diff.any(axis=1).sum())} points differ, first at {np.argwhere(diff)[0].tolist()}"


def test_the_cases_can_tell_a_division_from_a_multiplied_reciprocal(cases):
    """Of the reference alone: the focal lengths of the depth cases are not dyadic, and replacing the two divisions by a multiply with
    the rounded reciprocal changes points — so the comparison above (and the GPU's) would see that rule."""
    for name in ("depth_u16,100x72", "depth_u16,48x40", "depth_f32", "far,pitched"):
        c = cases[name]
        fx = float(c["im"]["fx"])
        assert np.frexp(fx)[0] != 0.5, name  # not a power of two
        wrong = ir.points(c["im"], c["image"], reciprocal=True)
        differ = (bits(wrong) != bits(c["points"])).any(axis=1)
        print(name, "fx", fx, "points that differ under the reciprocal rule:", int(differ.sum()))
        assert differ.sum() >= 1, name


def test_padding_and_steps_select_the_right_pixels(cases):
    """The pitched cases' padding is a valid depth that must never be read; the stepped cases are the plain ones' points, thinned."""
    a, b = cases["depth_u16,48x40"], cases["depth_u16,pitch+7"]
    assert b["image"].shape == (120, 167) and (b["image"][:, 160:] == ir.SENTINEL_U16).all() and np.array_equal(bits(a["points"]), bits(b["points"]))
    full, thin = cases["depth_u16,100x72"], cases["depth_u16,steps(2,3)"]
    want = full["points"].reshape(120, 160, 3)[::2, ::3].reshape(-1, 3)
    assert len(thin["points"]) == 60 * 54 and np.array_equal(bits(thin["points"]), bits(want))
    f = cases["depth_f32,steps(2,3),pitch+7"]
    assert f["image"].shape == (120, 167) and len(f["points"]) == 60 * 54


# ---- 3. refusals and valid edges ----------------------------------------------------------------------------------------------------
ROWS, COLS = 48, 40
GOOD = dict(model="pinhole", format="u16", width=8, height=6, depth_scale=0.001, fx=50.0, fy=50.0, cx=3.5, cy=2.5)
TABLES = dict(row_dir=np.ones((6, 2), F32), col_dir=np.ones((8, 2), F32))


def validate(im_kw=None, n_points=None, sp=None, cp=None, scan=None, im="make", roi=(0, 0, ROWS, COLS), stride=3):
    d = make_scan_image(**dict(GOOD, **(im_kw or {}))) if isinstance(im, str) else im
    if n_points is None and d is not None:
        nr, nc = scan_image_selected(d) if d.row_step >= 1 and d.col_step >= 1 else (d.height, d.width)
        n_points = nr * nc
    s = make_scan(np.eye(3, 4), n_points or 0, roi, stride) if scan is None else scan
    return scan_image_validate(ROWS, COLS, sr.RES, scan_params() if sp is None else sp, cp, s if scan != "null" else None, d)


def test_validate_accepts_the_valid_edges():
    assert validate() == OK
    assert validate(cp=scan_clear_params()) == OK
    assert validate(dict(width=4096, height=1)) == OK and validate(dict(width=1, height=4096)) == OK
    assert validate(dict(width=4096, height=1024)) == OK  # n_sel == FPE_SCAN_MAX_POINTS
    assert 4096 * 1024 == _capi.SCAN_MAX_POINTS == ir.MAX_POINTS
    assert validate(dict(width=4096, height=4096, row_step=2, col_step=2)) == OK  # the same count through the steps
    assert validate(dict(row_step=100, col_step=9)) == OK and validate(dict(row_step=2 ** 31 - 1, col_step=2 ** 31 - 1), n_points=1) == OK  # step > size
    assert validate(dict(row_pitch=8)) == OK and validate(dict(row_pitch=9)) == OK  # pitch == width
    assert validate(dict(model="spherical", **TABLES)) == OK
    assert validate(dict(model="spherical", fx=0.0, fy=np.nan, cx=np.inf, cy=np.nan, **TABLES)) == OK  # the intrinsics are the pinhole's
    assert validate(dict(row_dir=None, col_dir=None)) == OK  # the tables are the spherical model's
    assert validate(dict(fx=-50.0, fy=-1e-30, depth_scale=1e-38, format="f32")) == OK
    assert validate(stride=7) == OK  # point_stride passes the old check and is otherwise not read


BAD_IMAGES = dict(ir.REFUSED, **{
    "spherical without row_dir": dict(model="spherical", col_dir=TABLES["col_dir"]), "spherical without col_dir": dict(model="spherical", row_dir=TABLES["row_dir"]),
})


@pytest.mark.parametrize("what", list(BAD_IMAGES))
def test_validate_refuses_a_bad_descriptor(what):
    assert validate(BAD_IMAGES[what]) == BAD, what
    assert validate(BAD_IMAGES[what], cp=scan_clear_params()) == BAD, what


def test_validate_refuses_the_rest():
    for k in (0, 1):
        im = make_scan_image(**GOOD)
        im.reserved[k] = 1
        assert validate(im=im, n_points=48) == BAD, f"reserved[{k}]"
    assert validate(im=None, n_points=48) == BAD  # a null descriptor
    assert validate(scan="null") == BAD and scan_image_validate(ROWS, COLS, sr.RES, None, None, make_scan(np.eye(3, 4), 48, (0, 0, ROWS, COLS)), make_scan_image(**GOOD)) == BAD
    for n in (47, 49, 0, -1):
        assert validate(n_points=n) == BAD, f"n_points {n} against 48 selected pixels"
    assert validate(dict(row_step=2, col_step=3), n_points=48) == BAD and validate(dict(row_step=2, col_step=3), n_points=9) == OK
    # everything the point form refuses
    assert validate(stride=2) == BAD and validate(roi=(0, 0, 0, 5)) == BAD and validate(roi=(40, 0, 9, 5)) == BAD
    assert validate(scan=make_scan(np.where(np.arange(12) == 3, np.nan, np.eye(3, 4).reshape(12)), 48, (0, 0, ROWS, COLS))) == BAD
    assert validate(sp=scan_params(gate=0.0)) == BAD and validate(sp=scan_params(min_z=1.0, max_z=0.0)) == BAD
    for kw in (dict(sample_step=0.0), dict(min_hits=0), dict(ray_stride=0), dict(max_samples=65537), dict(reserved=7)):
        assert validate(cp=scan_clear_params(**kw)) == BAD, kw
    # a bad map geometry
    assert scan_image_validate(0, COLS, sr.RES, scan_params(), None, make_scan(np.eye(3, 4), 48, (0, 0, 1, 1)), make_scan_image(**GOOD)) != OK


def test_image_points_refuses_what_it_cannot_read():
    L = _capi.lib()
    img, out = np.ones(48, np.uint16), np.zeros((48, 3), F32)
    im = make_scan_image(**GOOD)
    assert L.fpe_scan_image_points(C.byref(im), _capi.ptr(img), _capi.ptr(out)) == OK
    assert L.fpe_scan_image_points(None, _capi.ptr(img), _capi.ptr(out)) == BAD
    assert L.fpe_scan_image_points(C.byref(im), None, _capi.ptr(out)) == BAD
    assert L.fpe_scan_image_points(C.byref(im), _capi.ptr(img), None) == BAD
    with pytest.raises(FpeError):
        scan_image_points(make_scan_image(**dict(GOOD, fx=0.0)), img)


# ---- 4. the ABI ---------------------------------------------------------------------------------------------------------------------
C_PROTOTYPES = {
    "fpe_scan_image_validate": "int (*)(const fpe_map_desc*, const fpe_scan_params*, const fpe_scan_clear_params*, const fpe_scan*, const fpe_scan_image*)",
    "fpe_scan_image_points": "int (*)(const fpe_scan_image*, const void*, float*)",
    "fpe_scan_fuse_image": "int (*)(fpe_scan_handle, const fpe_scan_params*, const fpe_scan*, const fpe_scan_image*, const void*, fpe_scan_info*)",
    "fpe_scan_fuse_image_device": "int (*)(fpe_scan_handle, const fpe_scan_params*, const fpe_scan*, const fpe_scan_image*, const void*, fpe_scan_info*, void*)",
    "fpe_scan_clear_image": "int (*)(fpe_scan_handle, const fpe_scan_params*, const fpe_scan_clear_params*, const fpe_scan*, const fpe_scan_image*, "
                            "const void*, fpe_scan_clear_info*)",
    "fpe_scan_clear_image_device": "int (*)(fpe_scan_handle, const fpe_scan_params*, const fpe_scan_clear_params*, const fpe_scan*, const fpe_scan_image*, "
                                   "const void*, fpe_scan_clear_info*, void*)",
    "fpe_scan_ingest_image": "int (*)(fpe_handle, fpe_scan_handle, const fpe_filter_params*, const fpe_scan_params*, const fpe_scan_clear_params*, "
                             "const fpe_scan_close_params*, const fpe_scan*, const fpe_scan_image*, const void*, const int32_t*, const double*, "
                             "fpe_scan_clear_info*, fpe_scan_info*, fpe_scan_close_info*, fpe_elevation_update_info*)",
    "fpe_scan_ingest_image_device": "int (*)(fpe_handle, fpe_scan_handle, const fpe_filter_params*, const fpe_scan_params*, const fpe_scan_clear_params*, "
                                    "const fpe_scan_close_params*, const fpe_scan*, const fpe_scan_image*, const void*, const int32_t*, const double*, "
                                    "fpe_scan_clear_info*, fpe_scan_info*, fpe_scan_close_info*, fpe_elevation_update_info*, void*)",
}


def test_the_c_side_of_the_abi(tmp_path):
    """The new declarations as a C99 host binds them (warnings as errors), the struct's size and the constants from a compiled probe;
    the ABI version stays 5; every new symbol is in the binding's table and in the library."""
    decls = "".join(f"  {proto.replace('(*)', f'(*p{k})')} = {name}; (void)p{k};\n" for k, (name, proto) in enumerate(C_PROTOTYPES.items()))
    body = ("  fpe_scan_image im = {FPE_SCAN_IMAGE_PINHOLE, FPE_SCAN_DEPTH_U16, 640, 480, 640, 1, 1, 0.001f, 500.0f, 500.0f, 319.5f, 239.5f, {0, 0}, 0, 0};\n"
            "  (void)im;\n"
            '  printf("%zu %zu %zu %d %d %d %d %d %d\\n", sizeof(fpe_scan_image), offsetof(fpe_scan_image, reserved), offsetof(fpe_scan_image, row_dir), '
            "FPE_ABI_VERSION, FPE_SCAN_IMAGE_PINHOLE, FPE_SCAN_IMAGE_SPHERICAL, FPE_SCAN_DEPTH_U16, FPE_SCAN_DEPTH_F32, FPE_SCAN_MAX_POINTS);")
    assert abi_c.compile_and_run(tmp_path, body, decls).split() == ["72", "48", "56", "5", "0", "1", "0", "1", str(1 << 22)]
    assert C.sizeof(_capi.ScanImage) == 72 and _capi.STRUCTS["fpe_scan_image"] is _capi.ScanImage and _capi.ABI_VERSION == 5
    assert (_capi.SCAN_IMAGE_PINHOLE, _capi.SCAN_IMAGE_SPHERICAL, _capi.SCAN_DEPTH_U16, _capi.SCAN_DEPTH_F32) == (0, 1, 0, 1)
    L = _capi.lib()
    assert L.fpe_abi_version() == 5
    for name in C_PROTOTYPES:
        assert name in _capi.PROTOTYPES and hasattr(L, name), name


# ---- 5. of the reference alone: each GPU case shows what it is there to show ---------------------------------------------------------
def info_of(case, **kw):
    return dict(zip(sr.INFO_FIELDS, ir.fuse(case, **kw)[2][:12].tolist()))


def test_the_depth_cases_show_every_drop_class_and_every_cell_class(cases):
    want = {"depth_u16,100x72": dict(cells_new=780, cells_fused=1526, cells_outlier=695, cells_replaced=220, below_band=688),
            "depth_u16,48x40": dict(cells_new=331, cells_fused=414, cells_outlier=239, cells_replaced=221)}
    for name, figures in want.items():
        c = cases[name]
        info = info_of(c)
        assert {k: info[k] for k in figures} == figures, name
        assert info["dropped_nonfinite"] == 2 and info["dropped_range"] == 2 and info["dropped_height"] == 1 and info["dropped_off_roi"] == 1, name
        # the state the scan itself leaves loses no cell to a clear of the same scan; a ghost goes; the prior's raised third goes
        own = cr.own_state(c)
        assert ir.clear(c, elev=own[0], var=own[1])[2]["cells_cleared"] == 0, name
    lost = {name: (int(ir.clear(cases[name], elev=cr.ghost_state(cases[name])[0], var=cr.ghost_state(cases[name])[1])[2]["cells_cleared"]),
                   int(ir.clear(cases[name])[2]["cells_cleared"])) for name in want}
    assert lost == {"depth_u16,100x72": (19, 435), "depth_u16,48x40": (20, 119)}
    f = info_of(cases["depth_f32"])
    assert f["dropped_nonfinite"] == 5 and min(f[k] for k in ("dropped_range", "dropped_height", "dropped_off_roi", "cells_new", "cells_fused",
                                                              "cells_outlier", "cells_replaced", "below_band")) > 0


def test_every_counter_of_the_clear(cases):
    for name in ("depth_u16,100x72", "far,pitched"):
        info = ir.clear(cases[name], cp=cr.params(**cr.EVERY_COUNTER))[2]
        assert min(int(info[k]) for k in ("strided_out", "dropped_points", "rays", "rays_long", "rays_empty", "cells_hit", "cells_cleared")) > 0, name


def test_the_lidar_cases_leave_the_map_and_drop_the_nan_column(cases):
    for name in ("lidar_f32,100x72", "lidar_f32,48x40"):
        c = cases[name]
        info = info_of(c)
        assert info["dropped_nonfinite"] == ir.RINGS and info["dropped_off_roi"] > 0 and info["accepted"] > 0, name  # one NaN table entry: a column
        assert np.isnan(c["points"].reshape(ir.RINGS, ir.AZIMUTHS, 3)[:, 5]).any(axis=1).all()
    info = info_of(cases["lidar_f32,100x72"])
    assert min(info[k] for k in ("cells_new", "cells_fused", "cells_outlier")) > 0
    assert ir.clear(cases["lidar_f32,100x72"])[2]["cells_cleared"] > 0


def test_the_far_case_is_far_and_pitched(cases):
    c = cases["far,pitched"]
    assert c["pos"] == sr.FAR_POS and info_of(c)["dropped_off_roi"] > 100 and info_of(c)["cells_replaced"] > 0


def test_the_contention_and_edge_cases(cases):
    one = cases["one cell"]
    f = ir.fuse(one)
    assert f[2][5] == 4096 and f[2][7] == 1 and f[3].max() > 64 and f[2][6] > 0  # one cell, more than 64 kept, some below the band
    assert np.unique(one["image"]).size == 4096 and np.ptp(one["image"].astype(int)) == 4095  # one raw unit apart
    row = ir.fuse(cases["one row"])
    assert row[2][5] == 64 and row[2][7] == 64 and row[3].max() == 1
    for w in ir.EDGE_WIDTHS:
        e = ir.fuse(cases[f"1x{w}"])
        assert e[2][0] == e[2][5] == w and (w < 63 or e[3].max() > 1)  # neighbouring pixels share cells
    for name, n in (("2x64,pitch70", 128), ("2x65,pitch70", 130)):
        c = cases[name]
        e = ir.fuse(c)
        assert c["im"]["row_pitch"] == 70 and e[2][5] == n and e[2][7] == 1  # one cell: its run spans the row end
