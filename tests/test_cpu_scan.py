"""The scan fusion's contract without a GPU (fpe_scan_*; include/fpe.h): the numpy statement (tests/scan_reference.py) against bytes
worked out by hand, its drop classes in their order of precedence, its independence of the order of the points, where points on cell
borders land (against the project's own host grid routines, tests/probe/scan_probe.cpp), fpe_scan_validate through ctypes, and the
conditions under which the GPU cases (tests/test_gpu_scan.py) show anything."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import make_scan, scan_params, scan_validate
from tests import scan_reference as sr

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def f32_bits(x):
    return np.asarray(x, F32).view(np.uint32)


# ---- 1. by hand --------------------------------------------------------------------------------------------------------------------
# A 4 x 4 map at 0.25 m about the origin: length 1, origin offset 0.5, first cell centre 0.375.  Cell (1, 2): centre (0.125, -0.125).
# The sensor frame is the map frame (T = identity, no translation): dx = 0.125, dy = -0.125, d2 = 0.03125.
# Three points at the cell's centre: z = 0.5, 0.53125, 0.25 -> q = 32768, 34816, 16384; top = 34816; band 0.125 -> band_q = 8192: the
# first two are kept (n = 2, S = 67584), the third lies below the band.  z_m = 33792 / 65536 = 0.515625.
# v_m = max((0.5 + 1.0 * 0.03125) / 2, 0) = 0.265625.
HAND_T = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)
HAND_POINTS = np.array([[0.125, -0.125, 0.5], [0.125, -0.125, 0.53125], [0.125, -0.125, 0.25]], F32)
HAND = dict(min_range=0.0, max_range=4.0, min_z=-1.0, max_z=1.0, band=0.125, var_base=0.5, var_range=1.0, var_min=0.0, var_max=8.0, gate=2.0,
            var_outlier=0.25)
# (prior h, prior v, replace_count) -> (h', v', class, info words 8..11)
HAND_CASES = {
    "NEW": (np.nan, np.nan, 0, 0.515625, 0.265625, 1, (1, 0, 0, 0)),
    # s = 0.53125, d = 0.015625, d*d << 4 s; k = 0.5: h' = 0.5 + 0.5 * 0.015625, v' = 0.265625 - 0.5 * 0.265625
    "FUSED": (0.5, 0.265625, 0, 0.5078125, 0.1328125, 2, (0, 1, 0, 0)),
    # d = -4: d*d = 16 > 4 * 0.53125; two kept points, replace_count 3: the prior stays, v' = 0.265625 + 0.25
    "OUTLIER": (4.515625, 0.265625, 3, 4.515625, 0.515625, 3, (0, 0, 1, 0)),
    # the same with replace_count 2: NEW's values
    "REPLACED": (4.515625, 0.265625, 2, 0.515625, 0.265625, 4, (0, 0, 1, 1)),
}


@pytest.mark.parametrize("name", list(HAND_CASES))
def test_hand_written_cell(name):
    h, v, rc, h2, v2, cls, counts = HAND_CASES[name]
    e0, v0 = sr.set_layers(np.full((4, 4), h, F32), np.full((4, 4), v, F32))
    e1, v1, info, cnt, cell_cls = sr.fuse(e0, v0, 0.25, (0.0, 0.0), sr.params(replace_count=rc, **HAND), HAND_T, HAND_POINTS, (0, 0, 4, 4))
    assert f32_bits(e1[1, 2]) == f32_bits(h2) and f32_bits(v1[1, 2]) == f32_bits(v2)
    assert cnt[1 * 4 + 2] == 2 and cell_cls[1 * 4 + 2] == cls
    assert info.tolist() == [3, 0, 0, 0, 0, 3, 1, 1, *counts, 1, 2, 1, 2]
    untouched = np.ones((4, 4), bool)
    untouched[1, 2] = False
    assert np.array_equal(sr.bits(e1)[untouched], sr.bits(e0)[untouched]) and np.array_equal(sr.bits(v1)[untouched], sr.bits(v0)[untouched])


def test_an_empty_scan_writes_nothing():
    e0, v0 = sr.unknown_layers(4, 4)
    e1, v1, info, _, _ = sr.fuse(e0, v0, 0.25, (0.0, 0.0), sr.params(**HAND), HAND_T, np.zeros((0, 3), F32), (0, 0, 4, 4))
    assert info.tolist() == [0] * 12 + [0, 0, -1, -1] and np.array_equal(sr.bits(e1), sr.bits(e0))


# ---- 2. drop classes, the earlier test first ---------------------------------------------------------------------------------------
def test_drop_classes_in_their_order_of_precedence():
    g = sr.geometry(4, 4, 0.25, (0.0, 0.0))
    p = sr.params(**HAND)
    pts = np.array([
        [np.nan, 0.0, 9.0],      # not finite (and out of range, too high): 0
        [0.0, np.inf, 0.0],      # 0
        [0.0, 0.0, 5.0],         # range (25 > 16), and too high, and ...: 1
        [3.0, 3.0, 0.0],         # range (18 > 16) and off the map: 1
        [0.0, 0.0, 2.0],         # in range (4 <= 16), too high: 2
        [2.0, 0.0, 1.5],         # too high and off the map: 2
        [0.7, 0.0, 0.0],         # off the map: 3
        [0.125, -0.125, 0.5],    # accepted in the whole map, off a roi of cell (0, 0): 4 / 3
        [0.5, 0.5, 0.0],         # exactly the map's first corner: t = 0 on both axes, inside, cell (0, 0)
        [-0.5, 0.0, 0.0],        # exactly the far edge: t = length, outside
    ], F32)
    cls, cell, q = sr.classify(g, p, HAND_T, pts, (0, 0, 4, 4))
    assert cls.tolist() == [0, 0, 1, 1, 2, 2, 3, 4, 4, 3]
    assert cell.tolist()[7:9] == [1 * 4 + 2, 0] and q.tolist()[7:9] == [32768, 0]
    cls, cell, _ = sr.classify(g, p, HAND_T, pts, (0, 0, 1, 1))
    assert cls.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 3] and cell[8] == 0
    # a range limit is compared as the double square of the float: |p|^2 = 16 exactly is in range, one ulp more is not
    edge = np.array([[4.0, 0.0, 0.0], [np.nextafter(F32(4.0), F32(5.0)), 0.0, 0.0]], F32)
    assert sr.classify(g, p, HAND_T, edge, (0, 0, 4, 4))[0].tolist() == [3, 1]


# ---- 3. permutation ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return sr.fuse_cases()


@pytest.fixture(scope="module")
def results(cases):
    return {name: sr.run(c) for name, c in cases.items()}


@pytest.mark.parametrize("name", ["100x72", "far,pitched"])
def test_permuting_the_points_changes_no_byte(cases, results, name):
    e, v, info, cnt, _ = results[name]
    for seed in (5, 6):
        e2, v2, info2, cnt2, _ = sr.run(cases[name], points=sr.shuffled(cases[name], seed))
        assert np.array_equal(sr.bits(e), sr.bits(e2)) and np.array_equal(sr.bits(v), sr.bits(v2))
        assert info.tolist() == info2.tolist() and np.array_equal(cnt, cnt2)


# ---- 4. cell borders ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    src, out = os.path.join(HERE, "probe", "scan_probe.cpp"), os.path.join(HERE, "probe", "_build", "libscan_probe.so")
    hdr = os.path.join(HERE, "..", "quadrupedal_foothold_planner_amd", "csrc", "fpe_gridmath.hpp")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(out):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src])
    L = C.CDLL(out)
    d = C.c_double
    L.scan_probe_cell.argtypes = [C.c_int, C.c_int, d, d, d, d, d, C.c_void_p]
    L.scan_probe_centre.argtypes = [C.c_int, C.c_int, d, d, d, C.c_int, C.c_int, C.c_void_p]
    return L


@pytest.mark.parametrize("res,pos", [(0.015625, (0.0, 0.0)), (0.015625, (1200.0, -41000.0)), (0.02, (0.0, 0.0)), (0.02, (0.3, -7.1))],
                         ids=["dyadic", "dyadic, far", "2 cm", "2 cm, off origin"])
def test_points_on_cell_borders_land_where_the_host_grid_routines_say(probe, res, pos):
    """Points on the borders between cells, and the float32 neighbours on either side (dyadic resolution: the borders are float32
    numbers, exactly; 2 cm: the nearest float32 numbers), through a pure translation by the map's position."""
    rows, cols = 48, 40
    g = sr.geometry(rows, cols, res, pos)
    T = np.hstack([np.eye(3), [[pos[0]], [pos[1]], [0.0]]]).reshape(12)
    ks = np.arange(-1, rows + 2)
    x = (g["orgX"] - ks * g["res"]).astype(F32)  # sensor frame = map frame moved by pos
    y = (g["orgY"] - (ks % (cols + 2)) * g["res"]).astype(F32)
    pts = np.concatenate([np.stack([f(x), f(y), np.full(len(ks), 0.5, F32)], axis=1)
                          for f in (lambda a: a, lambda a: np.nextafter(a, F32(np.inf)), lambda a: np.nextafter(a, F32(-np.inf)))])
    if res == 0.015625:
        assert np.array_equal(x.astype(np.float64), g["orgX"] - ks * g["res"])  # exactly on the borders
    cls, cell, _ = sr.classify(g, sr.params(min_range=0.0, max_range=100.0), T, pts, (0, 0, rows, cols))
    got = np.zeros(2, np.int32)
    n_in = 0
    for k, (px, py, _) in enumerate(pts.astype(np.float64)):
        inside = probe.scan_probe_cell(rows, cols, res, pos[0], pos[1], (1.0 * px + 0.0 * py) + pos[0], (0.0 * px + 1.0 * py) + pos[1], got.ctypes.data)
        inside = bool(inside) and 0 <= got[0] < rows and 0 <= got[1] < cols
        assert (cls[k] == 4) == inside, (k, px, py)
        if inside:
            assert cell[k] == got[0] * cols + got[1], (k, px, py)
            n_in += 1
    assert n_in > cols and (cls == 3).sum() >= 6
    # and the cell centres the variance model measures its distance to
    xy = np.zeros(2)
    for i, j in ((0, 0), (rows - 1, cols - 1), (17, 5)):
        probe.scan_probe_centre(rows, cols, res, pos[0], pos[1], i, j, xy.ctypes.data)
        assert xy[0] == sr.cell_pos(g["baseX"], g["res"], i) and xy[1] == sr.cell_pos(g["baseY"], g["res"], j)


# ---- 5. fpe_scan_validate ----------------------------------------------------------------------------------------------------------
ROWS, COLS = 100, 72
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def good_scan(**kw):
    s = make_scan(IDENT, 100, (10, 20, 30, 40))
    for k, v in kw.items():
        if k in ("roi", "reserved", "sensor_to_map"):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


def t_with(k, v):
    t = IDENT.reshape(12).copy()
    t[k] = v
    return list(t)


BAD_SCANS = {
    "n_points negative": dict(n_points=-1), "n_points above the cap": dict(n_points=_capi.SCAN_MAX_POINTS + 1),
    "stride 2": dict(point_stride=2), "stride 0": dict(point_stride=0), "reserved[0]": dict(reserved=[1, 0]), "reserved[1]": dict(reserved=[0, -1]),
    "roi without rows": dict(roi=[10, 20, 0, 40]), "roi without columns": dict(roi=[10, 20, 30, 0]), "roi of negative size": dict(roi=[10, 20, -3, 4]),
    "roi from a negative row": dict(roi=[-1, 0, 5, 5]), "roi from a negative column": dict(roi=[0, -1, 5, 5]),
    "roi past the last row": dict(roi=[71, 0, 30, 5]), "roi past the last column": dict(roi=[0, 33, 5, 40]),
    "roi whose end overflows": dict(roi=[2**31 - 1, 0, 2**31 - 1, 1]),
    "NaN in the rotation": dict(sensor_to_map=t_with(5, np.nan)), "infinite translation": dict(sensor_to_map=t_with(3, np.inf)),
}
BAD_PARAMS = {
    "min_range above max_range": dict(min_range=2.0, max_range=1.0), "min_z above max_z": dict(min_z=1.0, max_z=0.5),
    "max_z beyond 16384": dict(max_z=16385.0), "min_z beyond -16384": dict(min_z=-16400.0),
    "negative var_base": dict(var_base=-1e-9), "negative var_range": dict(var_range=-1.0), "negative var_min": dict(var_min=-1e-6),
    "negative var_max": dict(var_min=-2.0, var_max=-1.0), "negative var_outlier": dict(var_outlier=-0.1), "var_min above var_max": dict(var_min=2.0, var_max=1.0),
    "gate 0": dict(gate=0.0), "negative gate": dict(gate=-3.0), "negative band": dict(band=-0.01),
    **{f"{k} NaN": {k: np.nan} for k in ("min_range", "max_range", "min_z", "max_z", "band", "var_base", "var_range", "var_min", "var_max", "gate", "var_outlier")},
    "infinite max_range": dict(max_range=np.inf), "infinite var_max": dict(var_max=np.inf), "infinite band": dict(band=np.inf),
}


def test_validate_passes_the_defaults_and_the_valid_edges():
    sp = scan_params()
    assert {k: getattr(sp, k) for k, _ in _capi.ScanParams._fields_} == {k: (v if k == "replace_count" else F32(v)) for k, v in sr.DEFAULTS.items()}
    assert scan_validate(ROWS, COLS, 0.02, sp, good_scan()) == _capi.FPE_OK
    for kw in (dict(n_points=0), dict(n_points=_capi.SCAN_MAX_POINTS), dict(roi=[99, 71, 1, 1]), dict(roi=[0, 0, 1, 1]), dict(roi=[0, 0, ROWS, COLS]),
               dict(point_stride=3), dict(point_stride=16)):
        assert scan_validate(ROWS, COLS, 0.02, sp, good_scan(**kw)) == _capi.FPE_OK, kw
    for kw in (dict(max_z=16384.0, min_z=-16384.0), dict(min_range=1.0, max_range=1.0), dict(min_z=0.5, max_z=0.5), dict(var_min=0.0, var_max=0.0),
               dict(band=0.0), dict(var_base=0.0, var_range=0.0, var_outlier=0.0), dict(replace_count=1), dict(gate=1e-30)):
        assert scan_validate(ROWS, COLS, 0.02, scan_params(**kw), good_scan()) == _capi.FPE_OK, kw


@pytest.mark.parametrize("name", list(BAD_SCANS))
def test_validate_refuses_a_bad_scan(name):
    assert scan_validate(ROWS, COLS, 0.02, scan_params(), good_scan(**BAD_SCANS[name])) == _capi.FPE_E_INVALID_ARG


@pytest.mark.parametrize("name", list(BAD_PARAMS))
def test_validate_refuses_bad_parameters(name):
    assert scan_validate(ROWS, COLS, 0.02, scan_params(**BAD_PARAMS[name]), good_scan()) == _capi.FPE_E_INVALID_ARG


def test_validate_refuses_null_arguments_and_a_bad_geometry():
    L = _capi.lib()
    sp, s = scan_params(), good_scan()
    assert scan_validate(ROWS, COLS, 0.02, None, s) == _capi.FPE_E_INVALID_ARG
    assert scan_validate(ROWS, COLS, 0.02, sp, None) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_scan_validate(None, C.byref(sp), C.byref(s)) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_scan_params_defaults(None) == _capi.FPE_E_INVALID_ARG
    for rows, cols, res in ((0, COLS, 0.02), (ROWS, -1, 0.02), (ROWS, COLS, 0.0), (ROWS, COLS, np.nan)):
        assert scan_validate(rows, cols, res, sp, s) == _capi.FPE_E_INVALID_ARG
    # the roi is measured against THIS geometry
    assert scan_validate(39, 60, 0.02, sp, s) == _capi.FPE_E_INVALID_ARG and scan_validate(40, 59, 0.02, sp, s) == _capi.FPE_E_INVALID_ARG
    assert scan_validate(40, 60, 0.02, sp, s) == _capi.FPE_OK


def test_new_symbols_are_declared_bound_and_exported():
    import re

    with open(os.path.join(HERE, "..", "include", "fpe.h")) as f:
        declared = set(re.findall(r"^int (fpe_scan_\w+)\(", f.read(), re.M))
    assert len(declared) == 15 and declared <= set(_capi.PROTOTYPES)
    L = _capi.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert L.fpe_abi_version() == 5


# ---- 6. the GPU cases show something -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.fuse_cases()))
def test_gpu_fuse_cases_cover_every_class(cases, results, name):
    c = cases[name]
    e, v, info, cnt, cell_cls = results[name]
    assert len(c["points"]) <= 20000 and c["points"].shape[1] == c["stride"]
    f = dict(zip(sr.INFO_FIELDS, info.tolist()))
    assert all(f[k] >= 1 for k in ("dropped_nonfinite", "dropped_range", "dropped_height", "dropped_off_roi", "accepted", "below_band"))
    assert f["cells_new"] >= 1 and f["cells_fused"] >= 1 and f["cells_replaced"] >= 1 and f["cells_outlier"] > f["cells_replaced"]
    assert cnt.max() > 64
    assert f["n_points"] == len(c["points"]) == sum(f[k] for k in sr.INFO_FIELDS[1:6])
    assert f["cells_touched"] == f["cells_new"] + f["cells_fused"] + f["cells_outlier"] == int((cnt > 0).sum())
    # untouched cells inside the bounding box exist: a kernel that wrote them would show (the prior differs from cell to cell)
    r0, c0, r1, c1 = info[12:].tolist()
    assert (cell_cls.reshape(c["rows"], c["cols"])[r0:r1 + 1, c0:c1 + 1] == 0).any()
    same = sr.bits(e) == sr.bits(c["elev"])
    assert same.reshape(-1)[cell_cls == 0].all() and not same.reshape(-1)[np.isin(cell_cls, (1, 2, 4))].any()


def test_gpu_contention_roi_and_edge_cases_touch_cells(cases):
    c = cases["100x72"]
    for name, pts in sr.contention_cases(c).items():
        assert len(pts) <= 20000
        info, cnt = sr.run(c, points=pts)[2:4]
        assert info[5] == len(pts) and info[7] == {"one cell": 1, "one row": c["cols"], "one point per cell": c["rows"] * c["cols"]}[name], name
        assert cnt.max() == {"one cell": 4096, "one row": 57, "one point per cell": 1}[name]
    for name, roi in sr.roi_cases(c["rows"], c["cols"]).items():
        info = sr.run(c, roi=roi, points=sr.roi_points(c))[2]
        assert len(sr.roi_points(c)) <= 20000 and info[7] == roi[2] * roi[3], name
        assert name == "whole map" or info[4] > 1000, name  # the smaller rois drop what falls beside them
    # two fuses in a row with different rois: the second sees the first's result
    e1, v1 = sr.run(c, roi=sr.TWO_ROIS[0])[:2]
    info2 = sr.run(c, roi=sr.TWO_ROIS[1], elev=e1, var=v1, points=sr.shuffled(c, 9))[2]
    assert info2[9] >= 1 and info2[8] >= 1
    first_new = np.isnan(c["elev"]) & ~np.isnan(e1)  # cells the first fuse made known, inside the second roi: fused there, not new
    r0, c0, nr, nc = sr.TWO_ROIS[1]
    assert first_new[r0:r0 + nr, c0:c0 + nc].any()
