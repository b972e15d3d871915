"""One case per kernel form of the producer's filter chain: the table the CPU route test (tests/test_cpu_filter_route.py), the
oracle comparison (tests/test_gpu_filter_forms.py), the region launches (tests/test_gpu_elevation_update.py, section 9) and the
kernel trace (profiles/filter_form_kernels.txt) share.  Plain data and numpy helpers; the oracle runs on the CPU.

A form is what csrc/fpe_host.cpp::filter_route names for (geometry, parameters):
  first / second  a step window: (kind, TR, TC, HS) — kind 0 the walking kernel (filter_step1_kernel / filter_step2_kernel),
                  1 row runs filter_step_runs[_region]_kernel<.., TR, TC, HS>, 2 the second window rides in the fused launch
  fused           filter_fused[_region]_kernel<H, 32, TC, HS>; (0, 0, 0): the separate normals (and roughness) kernels
Every case's map is ragged in both axes for each tile shape its kernels use, and at most 160 x 96 cells.

The terrain of a case (terrain below) is made so that a wrong form shows: one riser across the map, ~1 % holes, cells of +-inf,
a hole in each map corner, a band of holes holding one line of finite cells of varying elevation (its discs are collinear:
rank-deficient and no plateau, so the cells walk) and a constant plateau with an edge — band and plateau away from tile (0, 0)
of every tile shape the case's kernels use (tests/test_gpu_elevation_update.py, section 8, places them the same way)."""
import functools
from collections import namedtuple

import numpy as np

from tests import elevation_update_reference as er

WALK, RUNS, IN_FUSED = 0, 1, 2
RIDES = (IN_FUSED, 0, 0, 0)
OFF = (123.456, -78.9)  # off the origin and off the lattice

FormCase = namedtuple("FormCase", "label rows cols res pos radii first fused second trav_only region_ok seed")


def both(r):
    return dict(normal_radius=r, roughness_radius=r)


def _c(label, rows, cols, res, radii, first, fused, second=RIDES, pos=(0.0, 0.0), seed=0):
    first = first if len(first) == 4 else (RUNS,) + first
    second = second if len(second) == 4 else (RUNS,) + second
    trav_only = int(fused != (0, 0, 0) and second == RIDES)
    return FormCase(label, rows, cols, res, pos, radii, first, fused, second, trav_only, int(trav_only and first[0] == RUNS), seed)


A, B, Cc = (100, 72, 0.02), (156, 92, 0.01), (124, 92, 0.005)
CASES = [
    # ---- the 14 fused forms <H, 32, TC, HS>; the first window is the published one (0.08 m): (32, 32, 5) at 2 cm, (32, 32, 9) at 1 cm
    _c("100x72@0.02 r=0.01", *A, both(0.01), (32, 32, 5), (1, 16, 0)),
    _c("100x72@0.02 r=0.03", *A, both(0.03), (32, 32, 5), (2, 16, 0)),
    _c("100x72@0.02 second=0.10", *A, dict(step_second_radius=0.10), (32, 32, 5), (3, 16, 0)),
    _c("100x72@0.02", *A, {}, (32, 32, 5), (3, 16, 5)),
    _c("100x72@0.02 r=0.07", *A, both(0.07), (32, 32, 5), (4, 16, 0)),
    _c("100x72@0.02 r=0.09", *A, both(0.09), (32, 32, 5), (5, 16, 0)),
    _c("100x72@0.02 r=0.11", *A, both(0.11), (32, 32, 5), (6, 16, 0)),
    _c("156x92@0.01", *B, {}, (32, 32, 9), (6, 16, 9)),
    _c("100x72@0.02 r=0.13", *A, both(0.13), (32, 32, 5), (7, 16, 0)),
    _c("156x92@0.01 r=0.075", *B, both(0.075), (32, 32, 9), (8, 16, 0)),
    _c("156x92@0.01 r=0.085 off origin", *B, both(0.085), (32, 32, 9), (9, 32, 0), pos=OFF),
    _c("156x92@0.01 r=0.095", *B, both(0.095), (32, 32, 9), (10, 32, 0)),
    _c("156x92@0.01 r=0.105", *B, both(0.105), (32, 32, 9), (11, 32, 0)),
    _c("156x92@0.01 r=0.115", *B, both(0.115), (32, 32, 9), (12, 32, 0)),
    # ---- the row-run forms (TR, TC, HS) as first window ((32, 32, 5) and (32, 32, 9): above)
    _c("100x72@0.02 first=0.10", *A, dict(step_first_radius=0.10), (32, 32, 0), (3, 16, 5)),
    _c("124x92@0.005 r=0.03 off origin", *Cc, both(0.03), (32, 16, 17), (7, 16, 0), pos=OFF),
    _c("124x92@0.005 r=0.03 first=0.10", *Cc, dict(both(0.03), step_first_radius=0.10), (32, 16, 0), (7, 16, 0)),
    _c("44x40@0.02 off origin", 44, 40, 0.02, {}, (16, 16, 0), (3, 16, 5), pos=OFF),
    # ---- ... and as second window, filter_step_runs_kernel<true, ..>; the first two run the separate normals and roughness kernels,
    # the last two are the two sides of tF + 2 h2 = 64 / 66 behind the 32-column fused tile
    _c("100x72@0.02 roughness=0.07", *A, dict(roughness_radius=0.07), (32, 32, 5), (0, 0, 0), (32, 32, 0)),
    _c("44x40@0.02 roughness=0.07", 44, 40, 0.02, dict(roughness_radius=0.07), (16, 16, 0), (0, 0, 0), (16, 16, 0)),
    _c("100x72@0.01 r=0.085 second=0.155", 100, 72, 0.01, dict(both(0.085), step_second_radius=0.155), (32, 32, 9), (9, 32, 0), (32, 16, 0)),
    _c("100x72@0.01 r=0.085 second=0.165", 100, 72, 0.01, dict(both(0.085), step_second_radius=0.165), (32, 32, 9), (9, 32, 0), (32, 16, 17)),
    # ---- the walking step kernels on a trusted lattice: a window of 23.2 cells has 15 classes of row half-widths, one more than
    # the row-run tables hold (tests/test_cpu_filter_route.py pins where that happens: radii of 23.0 .. 23.35 cells only)
    _c("124x92@0.005 r=0.03 first=0.116", *Cc, dict(both(0.03), step_first_radius=0.116), (WALK, 0, 0, 0), (7, 16, 0)),
    _c("124x92@0.005 r=0.03 second=0.116", *Cc, dict(both(0.03), step_second_radius=0.116), (32, 16, 17), (7, 16, 0), (WALK, 0, 0, 0)),
]
CASES = [c._replace(seed=200 + k) for k, c in enumerate(CASES)]
BY_LABEL = {c.label: c for c in CASES}
assert len(BY_LABEL) == len(CASES)
SECOND_FORMS = {(32, 32, 0), (16, 16, 0), (32, 16, 0), (32, 16, 17)}

# Section 9 of tests/test_gpu_elevation_update.py launches the region twins of these (the other forms with region_ok = 1 are in its
# own cases and SHAPES already), each with shift (5, 3)
REGION_LABELS = ("100x72@0.02 r=0.03", "100x72@0.02 r=0.09", "100x72@0.02 r=0.11", "156x92@0.01 r=0.095", "156x92@0.01 r=0.105")


def full_radii(case):
    return dict(er.DEFAULT_RADII, **case.radii)


def halos(case):
    """(hN, hR, h1, h2): filter_halo per radius."""
    p = full_radii(case)
    return tuple(er.halo(p[k], case.res) for k in ("normal_radius", "roughness_radius", "step_first_radius", "step_second_radius"))


def tile_shape(case):
    """The largest tile (rows, columns) among the case's launches: outside [0, rows) x [0, cols) no kernel of it is in its tile (0, 0)."""
    shapes = [w[1:3] for w in (case.first, case.second) if w[0] == RUNS]
    if WALK in (case.first[0], case.second[0]) or case.fused == (0, 0, 0):
        shapes.append((16, 16))  # the walking kernels and the separate normals / roughness kernels
    if case.fused != (0, 0, 0):
        shapes.append((32, case.fused[1]))
    return max(s[0] for s in shapes), max(s[1] for s in shapes)


def placement(case):
    """Where the band of holes, its line of finite cells and the plateau go: (band rows, band cols, line row, plateau rows, plateau cols),
    each a (start, stop) pair.  The band is as tall as the normals' disc on either side of the line, so the line's discs hold the line
    alone; line and plateau lie beyond the first tile's rows or columns for every tile shape of the case."""
    rows, cols = case.rows, case.cols
    TR, TC = tile_shape(case)
    hN = halos(case)[0]
    if rows >= 96:
        line = TR + hN + 2                                   # band and line in tile rows >= 1
        band = (line - hN, line + hN + 1)
        plateau_r = (band[1] + 4, min(rows - 6, band[1] + 4 + 22))
        return band, (TC // 2 + 2, cols - 6), line, plateau_r, (TC + 4, cols - 18)
    # 44 x 40: the plateau in tile columns >= 1 above, the band in tile rows >= 1 (of 32 x 16 and 16 x 16 tiles) below
    line = 32 + hN + 1
    return (line - hN, line + hN + 1), (TC + 1, cols - 2), line, (17, 30), (TC + 4, cols - 4)


@functools.lru_cache(maxsize=None)
def _terrain(label):
    case = BY_LABEL[label]
    rows, cols = case.rows, case.cols
    rng = np.random.default_rng(case.seed + 5000)
    # hills, one riser across the map, noise, ~1 % holes; er.terrain is made in cells for 2 cm: its heights scale with the resolution
    # (as they stand, its grades at 0.5 cm are beyond the critical slope everywhere)
    z = (er.terrain(rows, cols, case.seed, holes=0.01) * np.float32(case.res / 0.02)).astype(np.float32)
    (b0, b1), (c0, c1), line, (p0, p1), (q0, q1) = placement(case)
    z[p0:p1, q0:q1] = np.float32(0.25)                       # a plateau: the cells at its edge see two elevations
    z[b0:b1, c0:c1] = np.nan
    z[line, c0 + 1:c1 - 1] = (0.1 + 0.03 * np.sin(np.arange(c1 - c0 - 2) / 3.0)).astype(np.float32)
    z[0, 0] = z[0, cols - 1] = z[rows - 1, 0] = z[rows - 1, cols - 1] = np.nan
    for v in (np.inf, -np.inf, np.inf, -np.inf, np.inf):     # a handful of cells GridMap::isValid refuses as it does NaN
        i, j = b0, c0
        while b0 <= i < b1 and c0 <= j < c1:                 # (not in the band: its line stays whole)
            i, j = int(rng.integers(2, rows - 2)), int(rng.integers(2, cols - 2))
        z[i, j] = v
    z.setflags(write=False)
    return z


def terrain(case):
    """The case's elevation layer (read-only, made once)."""
    return _terrain(case.label)


def oracle_params(case):
    from oracle import fpo
    o, p = fpo.filter_defaults(), full_radii(case)
    o["normalRadius"], o["roughnessRadius"] = p["normal_radius"], p["roughness_radius"]
    o["stepFirstRadius"], o["stepSecondRadius"] = p["step_first_radius"], p["step_second_radius"]
    return o


@functools.lru_cache(maxsize=None)
def _oracle(label):
    from oracle import fpo
    case = BY_LABEL[label]
    ora = fpo.traversability_filters(terrain(case), case.res, position=case.pos, params=oracle_params(case))
    for a in ora.values():
        a.setflags(write=False)
    return ora


def oracle(case):
    """The oracle's eight layers for the case (read-only, computed once per process)."""
    return _oracle(case.label)


def walking_cells(case, ora):
    """Rank-deficient cells that are no plateau interior — normal_z == 1 with a step height other than 0 (NaN included: a lone
    member) — outside the first tile of the case's largest tile shape.  These cells take the literal walks."""
    TR, TC = tile_shape(case)
    with np.errstate(invalid="ignore"):
        deficient = (ora["normal_z"] == 1.0) & ~(ora["step_height"] == 0)
    deficient[:TR, :TC] = False
    return deficient


def check_inputs(case, ora):
    """The conditions on a case's input, on the oracle's output alone: the terrain is mostly valid and spans the planner's thresholds,
    cells walk outside the first tile, and for the wide discs finite cells lie within the halo of all four borders (the clipped
    windows are exercised)."""
    t = ora["traversability"]
    assert np.isfinite(t).mean() >= 0.8, (case.label, float(np.isfinite(t).mean()))
    if halos(case)[0] == 1:
        # a disc of less than one cell holds its centre alone: the published filters give the z axis (slope 1) and a roughness of
        # 0 / 0, which is no value below the critical one: 0.  The layer is (1 + step + 0) / 3 <= 2 / 3 in every cell, whatever the
        # terrain — it spans the planner's thresholds below that
        assert np.nanmin(t) < 0.5 < np.nanmax(t) <= np.float32(2.0 / 3.0) + 1e-6, (case.label, float(np.nanmin(t)), float(np.nanmax(t)))
    else:
        assert np.nanmin(t) < 0.5 < 0.9 < np.nanmax(t), (case.label, float(np.nanmin(t)), float(np.nanmax(t)))
    n_walk = int(walking_cells(case, ora).sum())
    assert n_walk >= 20, (case.label, n_walk)
    H = halos(case)[0]
    if H >= 9:
        ok = np.isfinite(t)
        assert ok[:H].any() and ok[-H:].any() and ok[:, :H].any() and ok[:, -H:].any(), case.label
    return n_walk
