"""Elevation-driven map updates without a GPU (fpe_filter_reach_cells, fpe_elevation_update_plan; include/fpe.h).

1. The engine's host arithmetic — reach R, the dirty set D, its size, the refusals — against the numpy statement of the contract
   (tests/elevation_update_reference.py) on every shift x patch set x map of the shared cases.
2. D is SUFFICIENT, shown on the oracle alone: outside D the oracle's traversability of the base, shifted, equals the oracle's
   traversability of the composed elevation at the moved position, byte for byte, NaN patterns included.
   RESOLUTION OF THE TRANSLATION CASES: 0.015625 m (dyadic).  At 0.02 m no seed was found for which the oracle alone satisfies
   this on all cases: its sums of rounded f64 cell positions move a last bit under translation (seeds 11 .. 18, 30 cases each:
   879 .. 1 493 cells outside D differ in the last place).  At a dyadic resolution cell positions and their differences are exact
   and the equality is exact.
   D is not arbitrarily generous: with normal and roughness radius 0.075 m at 0.025 m (0.075 / 0.025 = 2.9999999999999996 in
   double: halo 3, while the lattice offset (3, 0) lies ON the circle and is a member for some cells) and step radii of half a cell,
   R = 3 is the true reach: the equality holds with R and breaks with R - 1.  That case has shift (0, 0), so nothing is
   translated and the non-dyadic resolution is harmless."""
import ctypes as C

import numpy as np
import pytest

from oracle import fpo
from quadrupedal_foothold_planner_amd import _capi, build
from quadrupedal_foothold_planner_amd.planner import FpeError, _map_desc, elevation_update_plan, filter_reach_cells, make_map_update
from tests import elevation_update_reference as er
from tests import map_update_reference as mu


def filter_params(**overrides):
    fp = _capi.FilterParams()
    assert _capi.lib().fpe_filter_params_defaults(C.byref(fp)) == _capi.FPE_OK
    for k, v in overrides.items():
        setattr(fp, k, v)
    return fp


def oracle_filter_params(radii):
    o = fpo.filter_defaults()
    o["normalRadius"], o["roughnessRadius"] = radii["normal_radius"], radii["roughness_radius"]
    o["stepFirstRadius"], o["stepSecondRadius"] = radii["step_first_radius"], radii["step_second_radius"]
    return o


# ---- 1. the host arithmetic against the reference -------------------------------------------------------------------------------
def test_reach_cells():
    assert filter_reach_cells(0.02) == er.reach(0.02) == 10  # the defaults at 2 cm
    assert filter_reach_cells(0.01) == er.reach(0.01) == 18
    for res in (0.02, 0.01, 0.005, 0.025, 0.015625, 0.03):
        for radii in (er.DEFAULT_RADII, dict(normal_radius=0.07, roughness_radius=0.07, step_first_radius=0.08, step_second_radius=0.08),
                      dict(normal_radius=0.075, roughness_radius=0.075, step_first_radius=0.0125, step_second_radius=0.0125),
                      dict(normal_radius=0.05, roughness_radius=0.11, step_first_radius=0.02, step_second_radius=0.03)):
            assert filter_reach_cells(res, filter_params(**radii)) == er.reach(res, **radii), (res, radii)
    assert er.reach(0.025, normal_radius=0.075, roughness_radius=0.075, step_first_radius=0.0125, step_second_radius=0.0125) == 3
    L = _capi.lib()
    assert L.fpe_filter_reach_cells(None, 0.0) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_filter_reach_cells(None, float("nan")) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_filter_reach_cells(C.byref(filter_params(normal_radius=-1.0)), 0.02) == _capi.FPE_E_INVALID_ARG


def test_the_reference_dirty_set_is_the_literal_definition():
    """dirty_set builds D from lines and rectangles; here against the cell-by-cell dilation of C united with B."""
    for rows, cols, shift, name, R in ((48, 40, (5, 3), "eight", 10), (48, 40, (-7, 0), "tilecorner", 3), (33, 50, (0, -2), "overlap", 7),
                                       (48, 40, (0, 0), "corner", 10), (30, 30, (30, 0), "none", 4), (40, 36, (-3, 37), "interior", 5)):
        rects = er.patch_rects(name, rows, cols, shift)
        want = er.dilate(er.changed_set(rows, cols, shift, rects), R) | er.clipped_set(rows, cols, shift, R)
        assert np.array_equal(er.dirty_set(rows, cols, shift, rects, R), want), (rows, cols, shift, name)
    # the composed elevation is map_update_reference's
    e = er.terrain(23, 37, 5)
    pv = er.patch_values([(4, 5, 9, 11), (8, 9, 9, 20)], 6)
    want = mu.compose(e, e, (2, -3), [(r, c, v, v) for r, c, v in pv])[1]
    assert np.array_equal(er.compose_elevation(e, (2, -3), pv).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("rows,cols,res", er.MAPS, ids=lambda v: str(v))
def test_plan_agrees_with_the_reference(rows, cols, res):
    R = er.reach(res)
    seen_routes = set()
    for shift in er.shifts(rows, cols):
        for name in er.PATCH_SETS:
            rects = er.patch_rects(name, rows, cols, shift)
            info, mask = elevation_update_plan(rows, cols, res, shift, er.moved_position((0.0, 0.0), shift, res), rects)
            want = er.dirty_set(rows, cols, shift, rects, R)
            what = (rows, cols, shift, name)
            assert info["reach_cells"] == R, what
            assert np.array_equal(mask.astype(bool), want), what
            assert info["dirty_cells"] == int(want.sum()), what
            carried = abs(shift[0]) < rows and abs(shift[1]) < cols
            assert info["route"] == (0 if carried else 1), what  # the default chain at 2 cm and 1 cm is the traversability-only one
            seen_routes.add(info["route"])
            assert info["dirty_cells"] <= info["recomputed_cells"] <= rows * cols, what
            if info["route"] == 1:
                assert info["recomputed_cells"] == rows * cols, what
            else:  # whole tiles of at most 32 x 32 cells
                assert info["recomputed_cells"] <= er.grown_rect_cells(rows, cols, er.dirty_rects(rows, cols, shift, rects, R), 31), what
            # the info alone (no mask) says the same
            assert elevation_update_plan(rows, cols, res, shift, (0.0, 0.0), rects, want_mask=False)[0]["dirty_cells"] == info["dirty_cells"]
    assert seen_routes == {0, 1}


def test_plan_routes_and_parameters():
    # roughness radius != normal radius, and the published windows at 0.5 cm: the full chain
    for rows, cols, res, fp in ((100, 72, 0.02, filter_params(roughness_radius=0.07)), (128, 96, 0.005, None)):
        info, mask = elevation_update_plan(rows, cols, res, (5, 3), (0.0, 0.0), [(40, 30, 5, 5)], params=fp)
        radii = dict(er.DEFAULT_RADII, roughness_radius=0.07) if fp is not None else er.DEFAULT_RADII
        assert info["route"] == 1 and info["recomputed_cells"] == rows * cols
        assert np.array_equal(mask.astype(bool), er.dirty_set(rows, cols, (5, 3), [(40, 30, 5, 5)], er.reach(res, **radii)))
    # a generic fused instantiation (radius 0.07 at 2 cm): region launches
    fp = filter_params(normal_radius=0.07, roughness_radius=0.07)
    info, _ = elevation_update_plan(100, 72, 0.02, (5, 3), (0.0, 0.0), [(40, 30, 5, 5)], params=fp)
    assert info["route"] == 0 and info["reach_cells"] == 10
    # a map too far from the origin for the lattice forms: the full chain
    info, _ = elevation_update_plan(100, 72, 0.01, (1, 0), (3.0e3, 0.0), [])
    assert info["route"] == 1
    # radii beyond the stencil tables
    with pytest.raises(FpeError) as e:
        elevation_update_plan(100, 72, 0.005, (0, 0), (0.0, 0.0), [], params=filter_params(normal_radius=0.2))
    assert e.value.code == _capi.FPE_E_UNSUPPORTED


def _update(**changes):
    """A valid elevation update of a 40 x 50 map with two patches (row-major pitched, column-major pitched), then `changes`."""
    a = np.zeros(4096, np.float32)
    addr = a.ctypes.data
    u = make_map_update((3, -2), (0.5, -0.25), [(2, 3, 5, 7, None, addr, 9, 1), (10, 20, 6, 4, None, addr, 1, 8)])
    for k, v in changes.items():
        if k[:3] in ("p0_", "p1_"):
            setattr(u.patch[int(k[1])], k[3:], v)
        elif k in ("shift", "position"):
            getattr(u, k)[0], getattr(u, k)[1] = v
        else:
            setattr(u, k, v)
    u._keep = a
    return u


def _plan(u, rows=40, cols=50, res=0.02, fp=None, info=None, mask=None):
    d = _map_desc(rows, cols, res)
    return _capi.lib().fpe_elevation_update_plan(C.byref(d), C.byref(fp) if fp is not None else None, C.byref(u) if u is not None else None,
                                                 C.byref(info) if info is not None else None, mask.ctypes.data if mask is not None else None)


SOME = np.zeros(4, np.float32)
REFUSED_AND_NEIGHBOUR = {
    "a traversability pointer": (dict(p0_traversability=SOME.ctypes.data), dict(p0_traversability=None)),
    "n_patches above the limit": (dict(n_patches=9), dict(n_patches=2)),
    "negative n_patches": (dict(n_patches=-1), dict(n_patches=0)),
    "reserved set": (dict(reserved=1), dict(reserved=0)),
    "NaN position": (dict(position=(float("nan"), 0.0)), dict(position=(1.0, -1.0))),
    "infinite position": (dict(position=(0.0, float("inf"))), dict(position=(0.0, 0.0))),
    "no rows": (dict(p0_n_rows=0), dict(p0_n_rows=1)),
    "no columns": (dict(p1_n_cols=0), dict(p1_n_cols=1)),
    "negative row0": (dict(p0_row0=-1), dict(p0_row0=0)),
    "negative col0": (dict(p0_col0=-1), dict(p0_col0=0)),
    "one row past the last": (dict(p0_row0=36), dict(p0_row0=35)),
    "one column past the last": (dict(p0_col0=44), dict(p0_col0=43)),
    "null elevation": (dict(p0_elevation=None), dict()),
    "row pitch below n_cols": (dict(p0_row_stride=6), dict(p0_row_stride=7)),
    "column pitch below n_rows": (dict(p1_col_stride=5), dict(p1_col_stride=6)),
    "both strides above one": (dict(p0_row_stride=9, p0_col_stride=2), dict(p0_row_stride=9, p0_col_stride=1)),
    "zero strides": (dict(p0_row_stride=0, p0_col_stride=0), dict(p0_row_stride=7, p0_col_stride=1)),
    "negative stride": (dict(p0_row_stride=-9), dict(p0_row_stride=9)),
}


@pytest.mark.parametrize("name", list(REFUSED_AND_NEIGHBOUR))
def test_plan_refuses_and_accepts_the_nearest_neighbour(name):
    refused, accepted = REFUSED_AND_NEIGHBOUR[name]
    info = _capi.ElevationUpdateInfo(-5, -5, -5, -5)
    mask = np.full((40, 50), 7, np.uint8)
    assert _plan(_update(**refused), info=info, mask=mask) == _capi.FPE_E_INVALID_ARG
    assert (info.reach_cells, info.route, info.dirty_cells, info.recomputed_cells) == (-5, -5, -5, -5) and (mask == 7).all()  # nothing written
    assert _plan(_update(**accepted), info=info, mask=mask) == _capi.FPE_OK
    assert info.reach_cells == 10 and set(np.unique(mask)) <= {0, 1}


def test_plan_edges():
    L = _capi.lib()
    assert _plan(_update()) == _capi.FPE_OK  # info and mask may both be null
    assert _plan(None) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_elevation_update_plan(None, None, C.byref(_update()), None, None) == _capi.FPE_E_INVALID_ARG
    assert _plan(_update(), res=0.0) == _capi.FPE_E_INVALID_ARG and _plan(_update(), res=float("nan")) == _capi.FPE_E_INVALID_ARG
    assert _plan(_update(), fp=filter_params(step_first_radius=0.0)) == _capi.FPE_E_INVALID_ARG
    assert _plan(_update(), fp=filter_params(step_critical_cells=0)) == _capi.FPE_E_INVALID_ARG
    assert _plan(_update(), res=0.001) == _capi.FPE_E_UNSUPPORTED  # 0.08 m spans more cells than the stencil tables hold
    # a traversability pointer is refused in every used patch, looked at in none that is unused
    assert _plan(_update(p1_traversability=SOME.ctypes.data)) == _capi.FPE_E_INVALID_ARG
    assert _plan(_update(n_patches=1, p1_traversability=SOME.ctypes.data)) == _capi.FPE_OK
    # the same update is refused by fpe_update_map's validation (it wants both layers) and the other way round
    d = _map_desc(40, 50, 0.02)
    assert L.fpe_map_update_validate(C.byref(d), C.byref(_update())) == _capi.FPE_E_INVALID_ARG
    # without an engine: FPE_E_INVALID_ARG for a null handle, before anything else is looked at
    assert L.fpe_update_elevation(None, None, C.byref(_update()), None) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_update_elevation_device(None, None, C.byref(_update()), None, None) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_read_map_layers(None, SOME.ctypes.data, None) == _capi.FPE_E_INVALID_ARG
    assert L.fpe_read_map_layers_device(None, None, None, None) == _capi.FPE_E_INVALID_ARG
    blob = open(build.LIB_PATH, "rb").read()
    assert b"filter_fused_region_kernel" in blob and b"filter_step_runs_region_kernel" in blob  # in the gfx950 code object
    assert C.sizeof(_capi.ElevationUpdateInfo) == 24


# ---- 2. D is sufficient: the oracle alone ----------------------------------------------------------------------------------------
DYADIC = 0.015625
POS0 = (0.25, -0.5)  # dyadic too
# (on 48 x 40 the grown "interior" patch leaves no cell outside D: that map runs the other three sets)
SUFFICIENT_CASES = [(rows, cols, shift, name, seed) for rows, cols in ((100, 72), (48, 40)) for shift in ((5, 3), (-7, 0), (0, -2))
                    for name, seed in (("bands", 11), ("interior", 12), ("tilecorner", 11), ("none", 12)) if (rows, name) != (48, "interior")]


def outside_d_mismatches(rows, cols, res, shift, name, seed, radii, R, pos0):
    e0 = er.terrain(rows, cols, seed)
    rects = er.patch_rects(name, rows, cols, shift)
    es = er.compose_elevation(e0, shift, er.patch_values(rects, seed + 1))
    prm = oracle_filter_params(radii)
    t0 = fpo.traversability_filters(e0, res, position=pos0, params=prm)["traversability"]
    t1 = fpo.traversability_filters(es, res, position=er.moved_position(pos0, shift, res), params=prm)["traversability"]
    d = er.dirty_set(rows, cols, shift, rects, R)
    differ = er.shifted(t0, shift).view(np.uint32) != t1.view(np.uint32)  # (NaN patterns included: bit patterns)
    assert np.isnan(e0).any() and np.isnan(t1).any() and np.isfinite(t1).mean() > 0.5
    return int((differ & ~d).sum()), int((~d).sum()), int((differ & d).sum())


@pytest.mark.parametrize("rows,cols,shift,name,seed", SUFFICIENT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_outside_d_the_oracle_is_carried_by_the_shift(rows, cols, shift, name, seed):
    bad, outside, changed = outside_d_mismatches(rows, cols, DYADIC, shift, name, seed, er.DEFAULT_RADII, er.reach(DYADIC), POS0)
    assert outside > 0 and changed > 0  # the case shows something: cells outside D exist, and inside D the layer did change
    assert bad == 0, f"{bad} of {outside} cells outside D differ from the shifted base"


TIGHT = dict(normal_radius=0.075, roughness_radius=0.075, step_first_radius=0.0125, step_second_radius=0.0125)


@pytest.mark.parametrize("name", ["interior", "tilecorner"])
def test_the_reach_is_not_generous(name):
    """R - 1 is too small where the halo formula is tight (module docstring): the equality holds with R = 3 and breaks with 2."""
    R = er.reach(0.025, **TIGHT)
    assert R == 3
    bad, outside, _ = outside_d_mismatches(100, 72, 0.025, (0, 0), name, 11, TIGHT, R, (0.0, 0.0))
    assert bad == 0 and outside > 0
    bad, _, _ = outside_d_mismatches(100, 72, 0.025, (0, 0), name, 11, TIGHT, R - 1, (0.0, 0.0))
    assert bad > 0
