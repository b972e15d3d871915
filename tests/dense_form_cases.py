"""One case per kernel form, workgroup seam and chunk edge of the open-loop queries (fpe_search_legs, fpe_centroid_legs), the three
dense maps built from them (fpe_foothold_map, fpe_foothold_snap, fpe_centroid_map) and fpe_export_layers: the table the CPU
conditions (tests/test_cpu_dense_forms.py), the oracle comparison (tests/test_gpu_dense_forms.py) and the kernel trace
(profiles/dense_form_kernels.txt) share.  Plain data and numpy helpers; the oracle runs on the CPU.

A case names the ordered kernels its one call must launch — the code's own launch sites: every hipLaunchKernelGGL of
launch_search_legs, launch_centroid_legs (csrc/fpe_kernels.hip), launch_foothold_map (csrc/fpe_footmap.hpp),
launch_foothold_snap_bits, launch_foothold_snap_literal (csrc/fpe_footsnap.hpp) and launch_centroid_map
(csrc/fpe_centroidmap.hpp), under the names a kernel trace shows (template arguments written out, no blanks).

  group "select"  one case per selection: the constants derive_constants gives for (parameters, geometry) pick the form
  group "seam"    maps wider than one workgroup of the column-blocked kernels (1024 columns of the two bit-plane kernels, 256 of
                  cmap_code_kernel, the 32 x 64 tiles of footmap_height_kernel), every cell compared with the oracle
  group "chunk"   more than kSnapChunk = 2^18 cells through the literal snap chain: its second chunk"""
import functools
from collections import namedtuple

import numpy as np

from quadrupedal_foothold_planner_amd import _capi, synth

DenseCase = namedtuple("DenseCase", "label group entry rows cols res pos params tuning radius polygon roi n start kernels terrain seed "
                                    "compare")

SNAP_CHUNK = 1 << 18  # kSnapChunk
SEAMS = (1024, 1056)  # first column of the second workgroup of the bit-plane kernels: whole map / the region from word 1

S8M, S8, S64 = "search_legs_kernel<8,true>", "search_legs_kernel<8,false>", "search_legs_kernel<64,false>"
C8M, C8, C64 = "centroid_legs_kernel<8,true>", "centroid_legs_kernel<8,false>", "centroid_legs_kernel<64,false>"
Z8M, Z8, Z64 = "cmap_z_kernel<8,true>", "cmap_z_kernel<8,false>", "cmap_z_kernel<64,false>"
FLAGS_BITS, HEIGHT = "footmap_flags_bits_kernel", "footmap_height_kernel"
DIRECT_TABLE, DIRECT_LITERAL = "footmap_direct_kernel<true>", "footmap_direct_kernel<false>"
SNAP_BITS, SNAP_QUERIES, SNAP_CONVERT = "footsnap_bits_kernel", "footsnap_queries_kernel", "footsnap_convert_kernel"
CMAP_ROWS, CMAP_CODE = "cmap_rows_kernel", "cmap_code_kernel"
EXPORT = "layers_export_kernel"

# The promise: the launch sites named above, written out once.  tests/test_cpu_dense_forms.py holds the table to it.
LAUNCH_SITES = (S8M, S8, S64, C8M, C8, C64, DIRECT_LITERAL, FLAGS_BITS, DIRECT_TABLE, HEIGHT, SNAP_BITS, SNAP_QUERIES, SNAP_CONVERT,
                CMAP_ROWS, CMAP_CODE, Z8M, Z8, Z64)


def literal(search, chunks=1):
    """The literal snap chain: per chunk the queries, search_legs_kernel itself, the conversion."""
    return (SNAP_QUERIES, search, SNAP_CONVERT) * chunks


def _c(label, group, entry, rows, cols, res, kernels, params=None, tuning=None, radius=None, polygon="rectangle", roi=None, n=0,
       start=(0, 0), terrain="hostile", seed=0, compare="all", pos=(0.0, 0.0)):
    return DenseCase(label, group, entry, rows, cols, res, pos, dict(params or {}), dict(tuning or {}), radius, polygon, roi, n, start,
                     tuple(kernels), terrain, seed, compare)


def foot(rf, R=None):
    p = dict(footRadius=np.float32(rf))
    if R is not None:
        p["searchRadius"] = np.float32(R)
    return p


TIE_RF = np.float32(0.05)
TIE_RES = float(np.float64(TIE_RF)) / 3.0  # the lattice offset (3, 0) lies on the foot circle

# ---- selection: the open-loop queries and cmap_z_kernel; (resolution, params.searchRadius, the three kernels) ----------------------
_FORMS = [
    ("2cm R=0.1", 0.02, 0.1, (S8M, C8M, Z8M)),       # tileW 19, the yaml foot: the 3 x 3 variant
    ("1cm R=0.1", 0.01, 0.1, (S8, C8, Z8)),          # tileW 31, nFoot 9
    ("0.5cm R=0.1", 0.005, 0.1, (S64, C64, Z64)),    # tileW 55
    ("2cm R=0.3", 0.02, 0.3, (S64, C64, Z64)),       # tileW 39: midCellInside is set and must not matter
]
CASES = []
for _name, _res, _R, (_s, _cl, _z) in _FORMS:
    for _n in (1, 97):  # 97 = 32 * 3 + 1 = 4 * 24 + 1: the last workgroup of the 8-lane and of the 64-lane form is partly empty
        CASES.append(_c(f"search_legs {_name} n={_n}", "select", "search_legs", 90, 110, _res, (_s,), params=foot(0.02, _R), n=_n))
        CASES.append(_c(f"centroid_legs {_name} n={_n}", "select", "centroid_legs", 90, 110, _res, (_cl,), params=foot(0.02, _R), n=_n))
    CASES.append(_c(f"centroid_map {_name}", "select", "centroid_map", 90, 110, _res, (CMAP_ROWS, CMAP_CODE, _z), params=foot(0.02, _R)))
CASES += [
    # the largest reach of the dense centroid kernels: ceil(1.94 / 0.02) + 2 = 99 of kCmapMaxReach = 100 (the radius is the call's:
    # params.searchRadius sizes the z kernel's tile and stays the yaml one)
    _c("centroid_map 2cm R=1.94", "select", "centroid_map", 90, 110, 0.02, (CMAP_ROWS, CMAP_CODE, Z8M), radius=1.94),
    # ---- fpe_foothold_map ----
    _c("foothold_map 1cm rf=0.035", "select", "foothold_map", 70, 90, 0.01, (FLAGS_BITS, HEIGHT), params=foot(0.035)),
    _c("foothold_map 1cm rf=0.062", "select", "foothold_map", 70, 90, 0.01, (DIRECT_TABLE, HEIGHT), params=foot(0.062)),
    _c("foothold_map 1cm rf=0.065 table overflow", "select", "foothold_map", 70, 90, 0.01, (DIRECT_LITERAL,), params=foot(0.065)),
    _c("foothold_map rf=0.05 res=rf/3 lattice tie", "select", "foothold_map", 70, 90, TIE_RES, (DIRECT_LITERAL,), params=foot(TIE_RF)),
    _c("foothold_map 2cm rf=0", "select", "foothold_map", 70, 90, 0.02, (DIRECT_LITERAL,), params=foot(0.0)),
    _c("foothold_map 1cm rf=0.035 literal_discs", "select", "foothold_map", 70, 90, 0.01, (DIRECT_LITERAL,), params=foot(0.035),
       tuning=dict(literal_discs=1)),
    # ---- fpe_foothold_snap ----
    _c("foothold_snap 1cm rf=0.035 R=0.15", "select", "foothold_snap", 70, 90, 0.01, (HEIGHT, SNAP_BITS), params=foot(0.035, 0.15)),
    _c("foothold_snap 1cm rf=0.035 R=0.15 hexagon", "select", "foothold_snap", 70, 90, 0.01, literal(S64), params=foot(0.035, 0.15),
       polygon="hexagon"),
    _c("foothold_snap 1cm rf=0.035 R=0.15 literal_discs", "select", "foothold_snap", 70, 90, 0.01, literal(S64), params=foot(0.035, 0.15),
       tuning=dict(literal_discs=1)),
    _c("foothold_snap 2cm R=0.7 rings", "select", "foothold_snap", 70, 90, 0.02, literal(S64), radius=0.7),
    _c("foothold_snap 2^-5 R=0.125 rectangle tie", "select", "foothold_snap", 70, 90, 0.03125, literal(S8), radius=0.125),  # (rf < 0.9 res)
    _c("foothold_snap 1cm rf=0.062 no row intervals", "select", "foothold_snap", 70, 90, 0.01, literal(S64), params=foot(0.062)),
]

# ---- seams ---------------------------------------------------------------------------------------------------------------------------
_WIDE = dict(rows=40, cols=1100, res=0.01, params=foot(0.035, 0.15), terrain="wide", seed=77)
_REGION = (3, 40, 30, 1050)  # from word 1: 34 words, two workgroups, an unaligned first row; the workgroup seam at column 1056
_ALL_TEN = (FLAGS_BITS, HEIGHT, HEIGHT, SNAP_BITS, CMAP_ROWS, CMAP_CODE, Z64, EXPORT)
CASES += [
    _c("seam foothold_map 40x1100", "seam", "foothold_map", kernels=(FLAGS_BITS, HEIGHT), **_WIDE),
    _c("seam foothold_snap 40x1100", "seam", "foothold_snap", kernels=(HEIGHT, SNAP_BITS), **_WIDE),
    _c("seam centroid_map 40x1100", "seam", "centroid_map", kernels=(CMAP_ROWS, CMAP_CODE, Z64), **_WIDE),
    _c("seam foothold_map 40x1100 region", "seam", "foothold_map", kernels=(FLAGS_BITS, HEIGHT), roi=_REGION, **_WIDE),
    _c("seam foothold_snap 40x1100 region", "seam", "foothold_snap", kernels=(HEIGHT, SNAP_BITS), roi=_REGION, **_WIDE),
    _c("seam centroid_map 40x1100 region", "seam", "centroid_map", kernels=(CMAP_ROWS, CMAP_CODE, Z64), roi=_REGION, **_WIDE),
    # two cmap_code_kernel column blocks, five cmap_rows_kernel blocks; every rectangle (101 rows) covers several 32-row words
    _c("seam centroid_map 150x300 2cm R=1.0", "seam", "centroid_map", 150, 300, 0.02, (CMAP_ROWS, CMAP_CODE, Z8M), radius=1.0,
       terrain="hostile", seed=78),
    # footmap_height_kernel's 32 x 64 tiles (3 x 3 of them) with the widest halo a proved table has: footReach 6
    _c("seam foothold_map 70x140 1cm rf=0.062", "seam", "foothold_map", 70, 140, 0.01, (DIRECT_TABLE, HEIGHT), params=foot(0.062),
       terrain="mild", seed=79),
    # all ten layers of the wide map, a start index that wraps in both axes
    _c("seam export_layers 40x1100", "seam", "export_layers", kernels=_ALL_TEN, start=(7, 1029), **_WIDE),
]

# ---- chunks: 513 x 513 = 263 169 cells = 2^18 + 1025 -----------------------------------------------------------------------------------
_BIG = dict(rows=513, cols=513, res=0.02, terrain="rough", seed=80, compare="band")
CASES += [
    _c("chunk foothold_snap 513x513 literal_discs", "chunk", "foothold_snap", kernels=literal(S8, 2), tuning=dict(literal_discs=1), **_BIG),
    # the region's own cell 2^18 is (511, 1) of the region: the chunk edge moves one map row down
    _c("chunk foothold_snap 513x513 literal_discs region", "chunk", "foothold_snap", kernels=literal(S8, 2), tuning=dict(literal_discs=1),
       roi=(1, 0, 512, 513), **_BIG),
    _c("chunk foothold_snap 513x513 hexagon", "chunk", "foothold_snap", kernels=literal(S8M, 2), polygon="hexagon", **_BIG),
]

CASES = [c._replace(seed=c.seed or 300 + k) for k, c in enumerate(CASES)]
BY_LABEL = {c.label: c for c in CASES}
assert len(BY_LABEL) == len(CASES)


# ---- parameters, region, radius ------------------------------------------------------------------------------------------------------
def params_of(case):
    p = _capi.params_yaml()
    for k, v in case.params.items():
        p[k] = v
    return p


def region(case):
    return tuple(case.roi) if case.roi is not None else (0, 0, case.rows, case.cols)


def radius_of(case):
    """The search radius the call works with: its own argument, else params.searchRadius (f32)."""
    return float(np.float32(case.radius)) if case.radius is not None else float(params_of(case)["searchRadius"][0])


def max_search_radius(case):
    """What the entry point hands derive_constants as the largest search radius (fpe_engine.cpp: prepare_call and its callers)."""
    pr = float(params_of(case)["searchRadius"][0])
    if case.entry in ("foothold_snap", "search_legs"):
        return max(pr, radius_of(case))
    return pr  # the centroid method and the foothold map size their tile by params.searchRadius alone


# ---- terrain -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _terrain(kind, rows, cols, res, pos, seed):
    trav, elev = synth.rough_map(rows, cols, res, seed, position=pos, bad_frac=0.002 if kind == "mild" else 0.02)
    if kind == "wide":
        # rough_map as it is, plus at either seam column s two slabs of cells below both thresholds, each facing eight clean columns:
        # rows 0-17 left of the seam, rows 22-39 right of it.  The cells of a slab next to the seam find their nearest candidate
        # across it, and the clean cells facing a slab have foot discs that fail by cells of the other side alone.  And the map's last
        # stair strip is taken out of a third of the columns, so that rectangles of the centroid method end on rows that are not
        # blocked (its code 1)
        for s in SEAMS:
            trav[0:18, s - 6:s], trav[0:18, s:s + 8] = np.float32(0.5), np.float32(1.0)
            trav[22:40, s:s + 6], trav[22:40, s - 8:s] = np.float32(0.5), np.float32(1.0)
        trav[rows - 4:, cols // 3:2 * cols // 3] = np.float32(1.0)
    elif kind == "mild":
        # for the 121-cell disc: few cells below the thresholds, so that discs pass and fail; elevations >= 10, a NaN patch, +inf
        rng = np.random.default_rng(seed + 1)
        hi = rng.choice(rows * cols, size=rows * cols // 50, replace=False)
        elev.reshape(-1)[hi] = np.float32(10.0) + rng.uniform(0, 5, hi.size).astype(np.float32)
        elev.reshape(-1)[hi[:5]] = np.float32(10.0)
        trav[rows // 3:rows // 3 + 7, cols // 4:cols // 4 + 7] = np.nan
        elev[rows // 3:rows // 3 + 7, cols // 4:cols // 4 + 7] = np.nan
        trav[0, : cols // 2] = np.inf
        elev[5:9, 5:9] = np.float32(12.0)
    elif kind == "hostile":
        # NaN / -inf / +inf patches, elevations >= 10 (one exactly 10), discs with no height below 10, sparse candidates so that spirals
        # walk several rings, and bands of rows wholly below every threshold (every centroid case; cells without a foothold)
        rng = np.random.default_rng(seed + 1)
        trav[rng.uniform(size=trav.shape) < 0.06] = np.float32(0.5)
        hi = rng.choice(rows * cols, size=rows * cols // 50, replace=False)
        elev.reshape(-1)[hi] = np.float32(10.0) + rng.uniform(0, 5, hi.size).astype(np.float32)
        elev.reshape(-1)[hi[:5]] = np.float32(10.0)
        r0, c0 = rows // 3, cols // 4
        trav[r0:r0 + 7, c0:c0 + 7] = np.nan
        elev[r0:r0 + 7, c0:c0 + 7] = np.nan
        trav[rows // 2:rows // 2 + 3, cols // 2:cols // 2 + 5] = -np.inf
        trav[0, : cols // 2] = np.inf
        elev[5:9, 5:9] = np.float32(12.0)
        for b in range(rows // 5, rows, rows // 4):
            trav[b, :] = 0.0
            if b + 8 < rows:
                trav[b + 6:b + 8, cols // 3:] = 0.0
    trav.setflags(write=False)
    elev.setflags(write=False)
    return trav, elev


def terrain(case):
    """(traversability, elevation) of the case, made once and read-only; cases of one map share it."""
    return _terrain(case.terrain, case.rows, case.cols, case.res, tuple(case.pos), case.seed)


@functools.lru_cache(maxsize=None)
def _omap(kind, rows, cols, res, pos, seed):
    from oracle import fpo
    trav, elev = _terrain(kind, rows, cols, res, pos, seed)
    return fpo.OracleMap(trav, elev, res, position=pos)


def oracle_map(case):
    return _omap(case.terrain, case.rows, case.cols, case.res, tuple(case.pos), case.seed)


# ---- the cells a case compares -------------------------------------------------------------------------------------------------------
def chunk_edge_row(case):
    """Map row of the region's linear cell 2^18 (the first cell of the literal chain's second chunk)."""
    r0, _, _, nc = region(case)
    return r0 + SNAP_CHUNK // nc


@functools.lru_cache(maxsize=None)
def _cells(label):
    case = BY_LABEL[label]
    r0, c0, nr, nc = region(case)
    ii, jj = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")
    if case.compare == "all":
        cells = np.stack([ii.ravel(), jj.ravel()], axis=1)
    else:  # the four rows around the chunk edge, whole, plus 3 000 random cells of the region
        e = chunk_edge_row(case)
        band = (ii >= e - 2) & (ii <= e + 1)
        rng = np.random.default_rng(case.seed + 7)
        rnd = np.stack([rng.integers(r0, r0 + nr, 3000), rng.integers(c0, c0 + nc, 3000)], axis=1)
        cells = np.concatenate([np.stack([ii[band], jj[band]], axis=1), rnd])
    cells.setflags(write=False)
    return cells


def cells(case):
    """Canonical map cells [(i, j), ...] the case compares with the oracle."""
    return _cells(case.label)


# ---- queries of the open-loop cases ----------------------------------------------------------------------------------------------------
def query_points(case):
    """n centres: the first on a cell centre, the others anywhere on the map (a margin of two cells keeps them inside).  The open-loop
    cases sit at the origin."""
    assert tuple(case.pos) == (0.0, 0.0)
    rng = np.random.default_rng(case.seed + 11)
    lx, ly = case.rows * case.res, case.cols * case.res
    m = 2 * case.res
    pts = np.stack([rng.uniform(-0.5 * lx + m, 0.5 * lx - m, case.n), rng.uniform(-0.5 * ly + m, 0.5 * ly - m, case.n)], axis=1)
    ok, x, y = oracle_map(case).get_position(case.rows // 2, case.cols // 3)
    assert ok
    pts[0] = (x, y)
    return pts


def search_queries(case):
    """fpe_leg_query records: getSearchPolygon(centre, R), LU, RU, RD, LD."""
    pts, R = query_points(case), radius_of(case)
    q = np.zeros(case.n, dtype=_capi.QUERY_DTYPE)
    q["cx"], q["cy"], q["search_radius"], q["n_vertices"] = pts[:, 0], pts[:, 1], R, 4
    q["vx"][:, :4] = pts[:, :1] + np.array([R, R, -R, -R])
    q["vy"][:, :4] = pts[:, 1:] + np.array([0.5 * R, -0.5 * R, -0.5 * R, 0.5 * R])
    return q


def centroid_queries(case):
    pts = query_points(case)
    q = np.zeros(case.n, dtype=_capi.CENTROID_QUERY_DTYPE)
    q["cx"], q["cy"], q["search_radius"] = pts[:, 0], pts[:, 1], 0.0  # 0: params.searchRadius
    return q


# ---- the oracle, once per case ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(label):
    from tests import util
    case = BY_LABEL[label]
    omap, p = oracle_map(case), params_of(case)
    op = util.to_oracle_params(p)
    if case.entry == "search_legs":
        out = omap.search_legs(op, util.to_oracle_queries(search_queries(case)))
    elif case.entry == "centroid_legs":
        from tests.test_gpu_centroid_map import oracle_records
        pts = query_points(case)
        out = oracle_records(omap, p, pts[:, 0], pts[:, 1], np.full(case.n, radius_of(case)))
    elif case.entry == "foothold_map":
        from tests.test_gpu_foothold_map import oracle_cells
        out = oracle_cells(omap, p, cells(case))
    elif case.entry == "foothold_snap":
        from tests.test_gpu_foothold_snap import expected, queries
        kind = 0 if case.polygon == "rectangle" else 1
        out = expected(omap.search_legs(op, util.to_oracle_queries(queries(omap, cells(case), radius_of(case), kind))), cells(case))
    elif case.entry == "centroid_map":
        from tests.test_gpu_centroid_map import cell_centres, dense_expected, oracle_records
        xs, ys = cell_centres(omap, cells(case))
        out = dense_expected(oracle_records(omap, p, xs, ys, np.full(len(xs), radius_of(case))), cells(case))
    else:
        raise ValueError(case.entry)  # fpe_export_layers is held to the three dense calls, not to the oracle
    for a in (out if isinstance(out, tuple) else (out,)):
        a.setflags(write=False)
    return out


def oracle(case):
    """What the oracle gives for the case's cells or queries (read-only, computed once per process):
    search_legs / centroid_legs records; foothold_map (flags, height); foothold_snap (offset, source, z); centroid_map (code, offset, z)."""
    return _oracle(case.label)


# ---- conditions on the inputs, on the oracle alone ---------------------------------------------------------------------------------------
def seam_columns(case):
    """The seam columns inside the case's region (SEAMS[0] for the whole map, SEAMS[1] for the region from word 1)."""
    if case.cols <= SEAMS[0]:
        return ()
    return (SEAMS[1],) if case.roi is not None else (SEAMS[0],)


def discs_fed_across(case, seam):
    """(left, right): how many cells left / right of the seam column, within the region's rows, have a foot disc (circle_cells) with
    a finite cell below the default threshold and every such cell on the other side of the seam."""
    omap, p = oracle_map(case), params_of(case)
    rf, thr = float(p["footRadius"][0]), np.float32(p["defaultFootholdThreshold"][0])
    reach = int(np.ceil(rf / case.res)) + 1
    r0, _, nr, _ = region(case)
    n = [0, 0]
    for i in range(r0, r0 + nr):
        for j in range(seam - reach, seam + reach):
            ok, x, y = omap.get_position(i, j)
            assert ok
            disc = omap.circle_cells(x, y, rf, max_cells=8192)
            t = omap.trav[disc[:, 0], disc[:, 1]]
            below = disc[np.isfinite(t) & (t < thr)]
            if below.shape[0] == 0:
                continue
            other = (below[:, 1] >= seam) if j < seam else (below[:, 1] < seam)
            if other.all():
                n[0 if j < seam else 1] += 1
    return tuple(n)


def landings_across(case, seam):
    """(from the left, from the right): spiral landings of the oracle's snap whose cell and landing lie on different sides."""
    off, src, _ = oracle(case)
    j = cells(case)[:, 1]
    land = j + off[:, 1].astype(np.int64)
    spiral = src == 1
    return int((spiral & (j < seam) & (land >= seam)).sum()), int((spiral & (j >= seam) & (land < seam)).sum())


# ---- the one call of a case (tests/test_gpu_dense_forms.py, profiles/dense_form_kernels.py) ------------------------------------------------
def upload(planner, case):
    trav, elev = terrain(case)
    planner.gridmapCallback(trav, elev, case.res, position=case.pos)


def call(planner, case, **overrides):
    """The case's call on the map current in `planner` (upload() first), under the case's parameters and tuning; overrides replace
    fields of the case (tuning={} runs the same call without its switch)."""
    case = case._replace(**overrides)
    planner.params = params_of(case)
    with planner.tuning(**case.tuning):
        if case.entry == "search_legs":
            return planner.checkFoothold(search_queries(case))
        if case.entry == "centroid_legs":
            return planner.centroid_legs(centroid_queries(case))
        if case.entry == "foothold_map":
            return planner.foothold_map(roi=case.roi)
        if case.entry == "foothold_snap":
            return planner.foothold_snap(roi=case.roi, search_radius=case.radius, polygon=case.polygon)
        if case.entry == "centroid_map":
            return planner.centroid_map(roi=case.roi, search_radius=case.radius)
        if case.entry == "export_layers":
            return planner.export_layers(roi=case.roi, start_index=case.start)
    raise ValueError(case.entry)
