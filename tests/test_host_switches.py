"""CPU tests of the switches csrc/fpe_host.cpp::derive_constants sets from (parameters, map geometry), compiled for the
host through tests/probe/host_consts_probe.cpp.  The magnitude of the map's coordinates is an input to them: winH (which
kernel family runs), footRobust (proved foot-disc offset table or the literal bounding-box walk), footReach, midCellInside
and cornerEps.  The flip points are computed here from the formulas the file's comments state (tests/far_origin.py) and
both sides of each are asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd import build as fbuild
from tests import far_origin as fo

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "probe", "host_consts_probe.cpp")
OUT = os.path.join(HERE, "probe", "_build", "libhost_consts_probe.so")
CSRC = os.path.join(HERE, "..", "quadrupedal_foothold_planner_amd", "csrc")


@pytest.fixture(scope="module")
def probe():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("fpe_host.cpp", "fpe_host.hpp", "fpe_launch.hpp", "fpe_device.hpp", "fpe_gridmath.hpp")]
    if not os.path.exists(OUT) or max(os.path.getmtime(f) for f in deps) > os.path.getmtime(OUT):
        hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(fbuild.HIPCC))), "include")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                               "-I" + hip_include, "-o", OUT, SRC])
    L = C.CDLL(OUT)
    L.probe_plan_consts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_float, C.c_void_p, C.c_void_p]
    L.probe_plan_consts.restype = None
    return L


def consts(probe, rows, cols, res, pos, R=None, rf=None, maxleg=None):
    p = _capi.params_yaml()
    if R is not None:
        p["searchRadius"] = np.float32(R)
    if rf is not None:
        p["footRadius"] = np.float32(rf)
    out = np.zeros(6, np.int32)
    eps = np.zeros(1, np.float64)
    max_r = max(float(p["searchRadius"][0]), float(np.float32(maxleg or 0.0)))
    probe.probe_plan_consts(p.ctypes.data, rows, cols, res, float(pos[0]), float(pos[1]), C.c_float(max_r), out.ctypes.data, eps.ctypes.data)
    return dict(winH=int(out[0]), footRobust=int(out[1]), footReach=int(out[2]), midCellInside=int(out[3]), nFoot=int(out[4]), tileW=int(out[5]),
                cornerEps=float(eps[0]))


def test_yaml_foot_at_2cm_loses_its_offset_table_where_the_formula_says(probe):
    """f32(0.02) on 2 cm cells: the lattice offset (1, 0) is 1.79e-11 m^2 from the circle; tol reaches that at
    maxAbs = 8.2e4 m.  Below: one-cell table, the 13 x 13 bit window of R = f32(0.1) (rectangle reach ceil(5.00000007) = 6,
    candidates 5 + 0).  Above: no table, footReach = ceil(rf / res) + 1 = 2, winH = 0 — the literal walks and the
    direct kernels.  The headline configuration leaves the bit-window kernels there, silently but for this test."""
    rows, cols, res = 200, 180, 0.02
    assert abs(fo.foot_gap(0.02, res) - 1.788e-11) < 1e-13
    flip = fo.foot_robust_flip_posx(0.02, res, rows, cols)
    assert 8.0e4 < flip < 8.4e4
    below = dict(winH=6, footRobust=1, footReach=0, midCellInside=1, nFoot=1)
    above = dict(winH=0, footRobust=0, footReach=2, midCellInside=1, nFoot=0)
    for px, want in ((0.0, below), (1234.56, below), (0.5 * flip, below), (flip * (1 - 1e-9), below), (flip * (1 + 1e-9), above),
                     (2.0 * flip, above), (999000.0, above), (-0.5 * flip, below), (-2.0 * flip, above)):
        got = consts(probe, rows, cols, res, (px, 0.0))
        assert {k: got[k] for k in want} == want, (px, got)
    # the larger of the two axes decides: the same in y
    for py, want in ((0.5 * flip, below), (2.0 * flip, above)):
        got = consts(probe, rows, cols, res, (0.0, py + rows * res - cols * res))
        assert {k: got[k] for k in want} == want, (py, got)
    b, a = fo.yaml_foot_positions()
    assert consts(probe, rows, cols, res, b)["footRobust"] == 1 and consts(probe, rows, cols, res, a)["footRobust"] == 0


def test_search_radius_tie_row_where_the_formula_says(probe):
    """reach(R): a quotient R / res within `slack` of an integer takes one more row.  R = f32(0.1) at 2 cm is 7.45e-8
    cells ABOVE 5: ceil already gives 6 and the tie term gives round + 1 = 6 — no change at any magnitude below the guard,
    with a foot whose table stays proved (0.03: gap 1e-4 m^2).  R = f32(0.06) is 6.7e-8 cells BELOW 3: 3 rows until slack
    reaches that, at mag = 9.4e4 m, 4 from there on; with a one-cell foot (0.008) nothing else hides it."""
    rows, cols, res = 200, 180, 0.02
    mag, q = fo.reach_tie_flip_mag(0.1, res)
    assert 5.0 < q < 5.0000001 and 1.0e5 < mag < 1.1e5
    for px in (0.0, 0.5 * mag, mag, 2.0 * mag, 999000.0):
        got = consts(probe, rows, cols, res, (px, 0.0), R=0.1, rf=0.03)
        assert (got["winH"], got["footRobust"], got["footReach"]) == (6, 1, 1), (px, got)
    mag, q = fo.reach_tie_flip_mag(0.06, res)
    assert 2.9999999 < q < 3.0 and 9.0e4 < mag < 1.0e5
    rest = fo.mag_of(0.0, 0.0, rows, cols, res, 0.06, 0.008)
    for m, want in ((0.5 * mag, 3), (mag * (1 - 1e-6), 3), (mag * (1 + 1e-6), 4), (2.0 * mag, 4)):
        got = consts(probe, rows, cols, res, (m - rest, 0.0), R=0.06, rf=0.008)
        assert (got["winH"], got["footRobust"], got["footReach"], got["midCellInside"]) == (want, 1, 0, 0), (m, got)
        got = consts(probe, rows, cols, res, (0.0, -(m - rest)), R=0.06, rf=0.008)  # the sum of both axes counts
        assert got["winH"] == want, (m, got)


def test_matrix_rows_with_the_3cm_foot_keep_their_window_out_to_the_guard(probe):
    """tests/test_gpu_plan_matrix.py's rows with rf = 0.03 (gap 1e-4 m^2 at 2 cm: the table stays proved to 4e11 m) name
    the same window at every position below 1e6; cornerEps is the stated 128 eps mag / res + 1e-12."""
    from tests.test_gpu_plan_matrix import MATRIX

    picked = [r for r in MATRIX if r.rf == 0.03]
    assert [r.id for r in picked] == ["w7_gen", "w8_gen"]
    for r in picked:
        for pos in ((0.0, 0.0), fo.NEAR, (123456.789, -98765.4321), fo.FAR, fo.FAR_DYADIC, (999990.0, 0.0), (0.0, -999990.0)):
            got = consts(probe, r.rows, r.cols, r.res, pos, R=r.R, rf=r.rf, maxleg=r.maxleg)
            assert (got["winH"], got["footRobust"], got["footReach"]) == (r.winH, 1, 1), (r.id, pos, got)
            mag = fo.mag_of(pos[0], pos[1], r.rows, r.cols, r.res, max(r.R, r.maxleg or 0.0), r.rf)
            assert got["cornerEps"] == pytest.approx(128.0 * fo.EPS * mag / r.res + 1e-12, rel=1e-12)
            assert got["cornerEps"] < 1e-3  # far below half a cell at every pinned position


def test_mid_cell_inside_does_not_depend_on_the_position(probe):
    """midCellInside = (rf >= 0.9 res): the 11 % margin of its proof is argued for |coordinates| <= 1e6."""
    for pos in ((0.0, 0.0), fo.FAR, (999990.0, -999990.0)):
        assert consts(probe, 200, 180, 0.02, pos, rf=0.0181)["midCellInside"] == 1
        assert consts(probe, 200, 180, 0.02, pos, rf=0.0179)["midCellInside"] == 0
