"""The scan visibility clearing's contract without a GPU (fpe_scan_clear*; include/fpe.h): the numpy statement
(tests/scan_clear_reference.py) against a ray traced by hand, the properties a clearing must have on the scan tests' cases (a scan
clears nothing of the state it made itself, a ghost goes and nothing beside it does), its independence of the order of the points,
fpe_scan_clear_validate through ctypes, the ABI, and the conditions under which the GPU cases (tests/test_gpu_scan_clear.py) show
anything."""
import ctypes as C

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import make_scan, scan_clear_params, scan_clear_validate, scan_params
from tests import abi_c
from tests import scan_clear_reference as cr
from tests import scan_reference as sr

F32 = np.float32


# ---- 1. by hand --------------------------------------------------------------------------------------------------------------------
# A 4 x 16 map at 0.25 m about the origin: lengths 1 and 4, origin offsets 0.5 and 2; column j holds 2 - 0.25 (j + 1) < y <= 2 - 0.25 j,
# row 1 holds 0 < x <= 0.25.  The sensor frame is the map frame moved to the sensor's origin (0.125, 1.875, 2).  sample_step 0.5: step
# = 0.125.  Ray A ends at (0, -2, -2) in the sensor frame: dx = 0, m = 2, K = 16 (a power of two: every t, y, z is exact);
# start_samples 2, end_samples 4: k = 2 .. 11, y = 1.875 - 0.125 k, z = 2 - 0.125 k:
#     k      2      3      4     5      6     7      8    9      10    11
#     y      1.625  1.5    1.375 1.25   1.125 1.0    .875 .75    .625  .5
#     col    1      2      2     3      3     4      4    5      5     6
#     z      1.75   1.625  1.5   1.375  1.25  1.125  1.0  .875   .75   .625
# margin 0.125; the prior of row 1: col 1 unknown, col 2 1.75, col 3 2.0, col 4 1.0, col 5 1.0, col 6 0.5:
#     violates -      no     YES   YES    YES   no     no   no     YES   no     (k = 3: 1.75 < 1.75 and k = 9: 1.0 < 1.0 are false)
# so A counts once against each of the columns 2, 3 (two violating samples, one count) and 5.
# Ray B ends at (0, -1, -2): m = 1, K = 8, k = 2 .. 3: (y 1.625, col 1, z 1.5: unknown) and (y 1.5, col 2, z 1.25: 1.375 < 1.75 YES).
# min_hits 2: column 2 has two hits and is cleared; its neighbour column 3 stays at one.  The third point is a NaN.
HAND_T = np.hstack([np.eye(3), [[0.125], [1.875], [2.0]]]).reshape(12)
HAND_POINTS = np.array([[0.0, -2.0, -2.0], [0.0, -1.0, -2.0], [np.nan, 0.0, 0.0]], F32)
HAND_SP = dict(min_range=0.0, max_range=4.0, min_z=-1.0, max_z=3.0)
HAND_CP = dict(sample_step=0.5, margin=0.125, start_samples=2, end_samples=4, min_hits=2, ray_stride=1, max_samples=16)
HAND_ROW = {2: 1.75, 3: 2.0, 4: 1.0, 5: 1.0, 6: 0.5}


def hand_layers():
    e = np.full((4, 16), 3.0, F32)  # (everything else stands high: no ray of row 1 comes near it)
    e[1] = np.nan
    for col, h in HAND_ROW.items():
        e[1, col] = h
    return sr.set_layers(e, np.full((4, 16), 0.5, F32))


def test_hand_traced_rays():
    e0, v0 = hand_layers()
    g = sr.geometry(4, 16, 0.25, (0.0, 0.0))
    counters, rid, cell, z, cnt = cr.samples(g, sr.params(**HAND_SP), cr.params(**HAND_CP), HAND_T, HAND_POINTS, (0, 0, 4, 16))
    assert cnt.tolist() == [10, 2] and rid.tolist() == [0] * 10 + [1] * 2
    assert cell.tolist() == [16 + c for c in (1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 1, 2)]
    assert z.tolist() == [1.75, 1.625, 1.5, 1.375, 1.25, 1.125, 1.0, 0.875, 0.75, 0.625, 1.5, 1.25]
    e1, v1, info, hits = cr.clear(e0, v0, 0.25, (0.0, 0.0), sr.params(**HAND_SP), cr.params(**HAND_CP), HAND_T, HAND_POINTS, (0, 0, 4, 16))
    assert {int(k): int(hits[k]) for k in np.nonzero(hits)[0]} == {16 + 2: 2, 16 + 3: 1, 16 + 5: 1}
    assert cr.flat(info) == [3, 0, 1, 2, 0, 0, 3, 1, 1, 2, 1, 2, 12, 4]
    want_e, want_v = sr.bits(e0).copy(), sr.bits(v0).copy()
    want_e[1, 2] = want_v[1, 2] = sr.CLEARED
    assert np.array_equal(sr.bits(e1), want_e) and np.array_equal(sr.bits(v1), want_v)
    # min_hits 1: the three cells; max_samples 15: ray A is long and only B counts; end_samples 6: B has no sample left
    assert cr.clear(e0, v0, 0.25, (0.0, 0.0), sr.params(**HAND_SP), cr.params(**dict(HAND_CP, min_hits=1)), HAND_T, HAND_POINTS, (0, 0, 4, 16))[2][
        "cells_cleared"] == 3
    info = cr.clear(e0, v0, 0.25, (0.0, 0.0), sr.params(**HAND_SP), cr.params(**dict(HAND_CP, max_samples=15, end_samples=6)), HAND_T, HAND_POINTS,
                    (0, 0, 4, 16))[2]
    assert cr.flat(info) == [3, 0, 1, 2, 1, 1, 0, 0, 0, 0, -1, -1, 0, 0]
    # a roi of the columns 3 .. 15: column 2 is outside, the ray's samples there are not inside, nothing is cleared
    info = cr.clear(e0, v0, 0.25, (0.0, 0.0), sr.params(**HAND_SP), cr.params(**HAND_CP), HAND_T, HAND_POINTS, (1, 3, 1, 13))[2]
    assert (info["samples_in_roi"], info["hit_pairs"], info["cells_hit"], info["cells_cleared"]) == (7, 2, 2, 0)


def test_an_empty_scan_and_a_ray_straight_down():
    e0, v0 = hand_layers()
    info = cr.clear(e0, v0, 0.25, (0.0, 0.0), sr.params(**HAND_SP), cr.params(**HAND_CP), HAND_T, np.zeros((0, 3), F32), (0, 0, 4, 16))[2]
    assert cr.flat(info) == [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, -1, 0, 0]
    # dx = dy = 0: K = 0, no sample (and no division by K)
    info = cr.clear(e0, v0, 0.25, (0.0, 0.0), sr.params(**HAND_SP), cr.params(**dict(HAND_CP, start_samples=0, end_samples=0)), HAND_T,
                    np.array([[0.0, 0.0, -2.0]], F32), (0, 0, 4, 16))[2]
    assert cr.flat(info) == [1, 0, 0, 1, 0, 1, 0, 0, 0, 0, -1, -1, 0, 0]


# ---- 2. what a clearing must do on the scan tests' cases ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return sr.fuse_cases()


def cleared(before, after):
    return ~np.isnan(before) & np.isnan(after)


@pytest.mark.parametrize("name", ["100x72", "48x40", "100x72,stride4"])
def test_a_scan_clears_nothing_of_the_state_it_made_and_only_the_ghost_of_a_ghost_state(cases, name):
    c = cases[name]
    e, v = cr.own_state(c)
    e1, v1, info, _ = cr.run(c, elev=e, var=v)
    assert info["cells_cleared"] == 0 and info["hit_pairs"] == 0 and info["rays"] > 19000 and info["samples_in_roi"] > 300000
    assert np.array_equal(sr.bits(e1), sr.bits(e)) and np.array_equal(sr.bits(v1), sr.bits(v))
    ge, gv = cr.ghost_state(c)
    e2, v2, info, _ = cr.run(c, elev=ge, var=gv)
    gone = cleared(ge, e2)
    r0, c0, nr, nc = cr.ghost_box(c)
    assert gone[r0:r0 + nr, c0:c0 + nc].sum() >= 1
    gone[r0:r0 + nr, c0:c0 + nc] = False
    assert not gone.any() and np.array_equal(np.isnan(e2), np.isnan(v2))


def test_the_pitched_case_loses_the_whole_ghost(cases):
    """(Its pinhole_scan is a two-step fixed point, not a ray-caster: at 0.7 rad some of its hits are not lines of sight, so its own
    state is not free of clears; the ghost's 36 cells go.)"""
    c = cases["far,pitched"]
    ge, gv = cr.ghost_state(c)
    e2 = cr.run(c, elev=ge, var=gv)[0]
    r0, c0, nr, nc = cr.ghost_box(c)
    assert cleared(ge, e2)[r0:r0 + nr, c0:c0 + nc].all()


@pytest.mark.parametrize("name", list(sr.fuse_cases()))
def test_the_cases_own_prior_loses_cells_of_its_raised_third_only(cases, name):
    c = cases[name]
    e1, v1, info, hits = cr.run(c)
    gone = cleared(c["elev"], e1)
    assert info["cells_cleared"] == gone.sum() > 100 and not gone[: 2 * c["rows"] // 3].any()
    assert np.array_equal(sr.bits(e1)[~gone], sr.bits(c["elev"])[~gone]) and np.array_equal(sr.bits(v1)[~gone], sr.bits(c["var"])[~gone])
    assert (sr.bits(e1)[gone] == sr.CLEARED).all() and (sr.bits(v1)[gone] == sr.CLEARED).all()
    r0, c0, r1, c1 = info["bbox"].tolist()
    ii, jj = np.nonzero(gone)
    assert (r0, c0, r1, c1) == (ii.min(), jj.min(), ii.max(), jj.max())


@pytest.mark.parametrize("name", ["100x72", "far,pitched"])
def test_permuting_the_points_changes_no_byte(cases, name):
    c = cases[name]
    e, v, info, hits = cr.run(c)
    for seed in (5, 6):
        e2, v2, info2, hits2 = cr.run(c, points=sr.shuffled(c, seed))
        assert np.array_equal(sr.bits(e), sr.bits(e2)) and np.array_equal(sr.bits(v), sr.bits(v2))
        assert info.tobytes() == info2.tobytes() and np.array_equal(hits, hits2)


# ---- 3. fpe_scan_clear_validate ------------------------------------------------------------------------------------------------------
ROWS, COLS = 100, 72
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])
BAD_CLEAR = {
    "sample_step 0": dict(sample_step=0.0), "negative sample_step": dict(sample_step=-0.5), "sample_step above 1": dict(sample_step=1.0000001),
    "sample_step NaN": dict(sample_step=np.nan), "sample_step infinite": dict(sample_step=np.inf), "negative margin": dict(margin=-1e-6),
    "margin NaN": dict(margin=np.nan), "margin infinite": dict(margin=np.inf), "negative start_samples": dict(start_samples=-1),
    "negative end_samples": dict(end_samples=-1), "min_hits 0": dict(min_hits=0), "negative min_hits": dict(min_hits=-2), "ray_stride 0": dict(ray_stride=0),
    "negative ray_stride": dict(ray_stride=-1), "max_samples 0": dict(max_samples=0), "max_samples 65537": dict(max_samples=65537),
    "negative max_samples": dict(max_samples=-4096), "reserved": dict(reserved=1),
}


def good_scan(**kw):
    s = make_scan(IDENT, 100, (10, 20, 30, 40))
    for k, v in kw.items():
        if k in ("roi", "reserved", "sensor_to_map"):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


def test_validate_passes_the_defaults_and_the_valid_edges():
    cp = scan_clear_params()
    assert {k: getattr(cp, k) for k, _ in _capi.ScanClearParams._fields_} == cr.params()
    assert scan_clear_validate(ROWS, COLS, 0.02, scan_params(), cp, good_scan()) == _capi.FPE_OK
    for kw in (dict(sample_step=1.0), dict(sample_step=1e-30), dict(margin=0.0), dict(start_samples=0), dict(end_samples=0), dict(start_samples=0, end_samples=0),
               dict(max_samples=1), dict(max_samples=65536), dict(min_hits=1), dict(min_hits=2**31 - 1), dict(ray_stride=2**31 - 1),
               dict(start_samples=2**31 - 1, end_samples=2**31 - 1)):
        assert scan_clear_validate(ROWS, COLS, 0.02, scan_params(), scan_clear_params(**kw), good_scan()) == _capi.FPE_OK, kw
    with pytest.raises(ValueError):
        scan_clear_params(no_such_field=1)


@pytest.mark.parametrize("name", list(BAD_CLEAR))
def test_validate_refuses_bad_clear_parameters(name):
    assert scan_clear_validate(ROWS, COLS, 0.02, scan_params(), scan_clear_params(**BAD_CLEAR[name]), good_scan()) == _capi.FPE_E_INVALID_ARG


def test_validate_refuses_what_the_fuse_refuses_and_null_arguments():
    L = _capi.lib()
    sp, cp, s = scan_params(), scan_clear_params(), good_scan()
    for bad in (dict(n_points=-1), dict(n_points=_capi.SCAN_MAX_POINTS + 1), dict(point_stride=2), dict(reserved=[0, 1]), dict(roi=[10, 20, 0, 40]),
                dict(roi=[71, 0, 30, 5]), dict(sensor_to_map=[np.nan] + [0.0] * 11)):
        assert scan_clear_validate(ROWS, COLS, 0.02, sp, cp, good_scan(**bad)) == _capi.FPE_E_INVALID_ARG, bad
    for bad in (dict(gate=0.0), dict(min_z=1.0, max_z=0.5), dict(max_z=16385.0), dict(band=np.nan), dict(min_range=2.0, max_range=1.0), dict(var_min=-1.0)):
        assert scan_clear_validate(ROWS, COLS, 0.02, scan_params(**bad), cp, s) == _capi.FPE_E_INVALID_ARG, bad
    assert scan_clear_validate(ROWS, COLS, 0.02, None, cp, s) == _capi.FPE_E_INVALID_ARG
    assert scan_clear_validate(ROWS, COLS, 0.02, sp, None, s) == _capi.FPE_E_INVALID_ARG
    assert scan_clear_validate(ROWS, COLS, 0.02, sp, cp, None) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_scan_clear_validate(None, C.byref(sp), C.byref(cp), C.byref(s)) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_scan_clear_params_defaults(None) == _capi.FPE_E_INVALID_ARG
    for rows, cols, res in ((0, COLS, 0.02), (ROWS, COLS, 0.0), (39, 60, 0.02)):
        assert scan_clear_validate(rows, cols, res, sp, cp, s) == _capi.FPE_E_INVALID_ARG
    assert scan_clear_validate(40, 60, 0.02, sp, cp, s) == _capi.FPE_OK


# ---- 4. the ABI ----------------------------------------------------------------------------------------------------------------------
CLEAR_SYMBOLS = ("fpe_scan_clear_params_defaults", "fpe_scan_clear_validate", "fpe_scan_clear", "fpe_scan_clear_device", "fpe_scan_ingest_clear",
                 "fpe_scan_ingest_clear_device")


def test_struct_layouts_against_the_c_compiler(tmp_path):
    pf = [k for k, _ in _capi.ScanClearParams._fields_]
    inf = list(_capi.SCAN_CLEAR_INFO_DTYPE.names)
    body = '  printf("%d %d %d\\n", (int)sizeof(fpe_scan_clear_params), (int)sizeof(fpe_scan_clear_info), FPE_ABI_VERSION);\n'
    body += "".join(f'  printf("{k} %d\\n", (int)offsetof(fpe_scan_clear_params, {k}));\n' for k in pf)
    body += "".join(f'  printf("{k} %d\\n", (int)offsetof(fpe_scan_clear_info, {k}));\n' for k in inf)
    decls = ("  fpe_scan_clear_params cp; fpe_scan_clear_info ci;\n"
             "  (void)fpe_scan_clear_params_defaults(&cp); (void)fpe_scan_clear_validate(0, 0, &cp, 0); (void)fpe_scan_clear(0, 0, &cp, 0, 0, &ci);\n"
             "  (void)fpe_scan_clear_device(0, 0, &cp, 0, 0, &ci, 0); (void)fpe_scan_ingest_clear(0, 0, 0, 0, &cp, 0, 0, 0, 0, &ci, 0, 0);\n"
             "  (void)fpe_scan_ingest_clear_device(0, 0, 0, 0, &cp, 0, 0, 0, 0, &ci, 0, 0, 0);\n")
    out = abi_c.compile_and_run(tmp_path, body, decls).split("\n")
    assert out[0] == "32 64 5"
    got = dict(line.split() for line in out[1:] if line)
    want = {k: str(getattr(_capi.ScanClearParams, k).offset) for k in pf}
    assert [want[k] for k in pf] == ["0", "4", "8", "12", "16", "20", "24", "28"]
    want.update({k: str(_capi.SCAN_CLEAR_INFO_DTYPE.fields[k][1]) for k in inf})
    assert got == want and want["bbox"] == "32" and want["samples_in_roi"] == "48" and want["hit_pairs"] == "56"
    # the reference's own record has the same layout
    assert cr.INFO_DTYPE.names == _capi.SCAN_CLEAR_INFO_DTYPE.names and all(cr.INFO_DTYPE.fields[k][:2] == _capi.SCAN_CLEAR_INFO_DTYPE.fields[k][:2] for k in inf)
    assert C.sizeof(_capi.ScanClearParams) == 32 and _capi.SCAN_CLEAR_INFO_DTYPE.itemsize == 64


def test_new_symbols_are_bound_and_exported_and_the_abi_version_stays():
    L = _capi.lib()
    for name in CLEAR_SYMBOLS:
        assert name in _capi.PROTOTYPES and name in _capi.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert L.fpe_abi_version() == 5 == _capi.ABI_VERSION
    assert _capi.STRUCTS["fpe_scan_clear_params"] is _capi.ScanClearParams and _capi.STRUCTS["fpe_scan_clear_info"] is _capi.SCAN_CLEAR_INFO_DTYPE


# ---- 5. the GPU cases show something -------------------------------------------------------------------------------------------------
def test_one_gpu_case_has_every_per_point_counter_above_zero(cases):
    c = cases["100x72"]
    info, hits = cr.run(c, cp=cr.params(**cr.EVERY_COUNTER))[2:]
    assert all(info[k] > 0 for k in ("strided_out", "dropped_points", "rays_long", "rays_empty", "cells_hit", "cells_cleared", "hit_pairs"))
    assert info["rays"] > info["rays_long"] + info["rays_empty"]
    assert info["n_points"] == len(c["points"]) == info["strided_out"] + info["dropped_points"] + info["rays"]


@pytest.mark.parametrize("name", list(sr.fuse_cases()))
def test_gpu_cases_hold_cells_at_and_just_below_min_hits_unknown_cells_and_long_rays(cases, name):
    c = cases[name]
    g = sr.geometry(c["rows"], c["cols"], c["res"], c["pos"])
    cp = cr.params()
    info, hits = cr.run(c)[2:]
    assert (hits == cp["min_hits"]).any() and (hits == cp["min_hits"] - 1).any() and (hits > 64).any()
    assert info["hit_pairs"] == hits.sum() and info["cells_hit"] == (hits > 0).sum() > info["cells_cleared"] == (hits >= cp["min_hits"]).sum()
    counters, rid, cell, z, cnt = cr.samples(g, c["params"], cp, c["T"], c["points"], c["roi"])
    assert cnt.max() > 64  # the group form crosses a chunk, at every group width
    ins = cell >= 0
    assert np.isnan(c["elev"].reshape(-1)[cell[ins]]).any()  # samples over unknown cells (the whole-map roi: local index = state index)
    assert len(c["points"]) <= 20000 and info["samples_in_roi"] <= 1500000


def test_gpu_roi_and_grazing_cases_cross_a_roi_they_do_not_end_in(cases):
    c = cases["100x72"]
    pts = sr.roi_points(c)
    for name, roi in sr.roi_cases(c["rows"], c["cols"]).items():
        info = cr.run(c, points=pts, roi=roi)[2]
        assert info["samples_in_roi"] > 0 and info["rays"] > 19000, name
    info = cr.run(c, points=pts, roi=sr.roi_cases(c["rows"], c["cols"])["ragged corner"])[2]
    assert info["cells_cleared"] > 0
    # rays that end beyond the map: none of the points is accepted by a fuse, every one crosses the map, and the raised third loses cells
    gp = cr.grazing_points(c)
    assert sr.run(c, points=gp)[2][5] == 0
    e1, _, info, hits = cr.run(c, points=gp, cp=cr.params(min_hits=1))
    assert info["rays"] == len(gp) and info["rays_long"] == 0 and info["samples_in_roi"] > 64 * len(gp) and info["cells_cleared"] > 0
    # the two rois in a row: the second clear sees what the first left
    e1, v1, info1, _ = cr.run(c, roi=sr.TWO_ROIS[0])
    info2 = cr.run(c, roi=sr.TWO_ROIS[1], elev=e1, var=v1, points=sr.shuffled(c, 9))[2]
    assert info1["cells_cleared"] > 0 and info2["cells_cleared"] > 0
    assert info2.tobytes() != cr.run(c, roi=sr.TWO_ROIS[1], points=sr.shuffled(c, 9))[2].tobytes()


def test_gpu_contention_cases_pile_rays_on_few_cells(cases):
    c = cases["100x72"]
    e, v = cr.raised(c)
    for name, pts in sr.contention_cases(c).items():
        info, hits = cr.run(c, points=pts, elev=e, var=v, cp=cr.params(**cr.CONTENTION))[2:]
        assert info["rays"] == len(pts) and info["rays_empty"] == 0 and info["rays_long"] == 0, name
        if name == "one cell":
            assert hits.max() == 4096 and info["cells_hit"] <= 8
        if name == "one point per cell":
            assert info["cells_cleared"] > 1000
