"""Plain numpy statement of the scan fusion (fpe_scan_fuse*, fpe_scan_move; include/fpe.h), written from the contract: the per-point
tests in f64, the per-cell integer reductions (np.maximum.at / np.add.at on int64), the f32 fusion rule, and the cases the CPU and the
GPU tests share.  Every product and sum is one numpy operation, so each is rounded on its own.  numpy only; no engine code."""
import numpy as np

CLEARED = np.uint32(0x7FC00000)
INFO_FIELDS = ("n_points", "dropped_nonfinite", "dropped_range", "dropped_height", "dropped_off_roi", "accepted", "below_band",
               "cells_touched", "cells_new", "cells_fused", "cells_outlier", "cells_replaced")
DEFAULTS = dict(min_range=0.1, max_range=10.0, min_z=-100.0, max_z=100.0, band=0.05, var_base=1e-4, var_range=1e-4, var_min=1e-6,
                var_max=1.0, gate=3.0, var_outlier=1e-3, replace_count=0)
F32, F64 = np.float32, np.float64


def params(**overrides):
    """The defaults of fpe_scan_params_defaults with any field replaced; floats as float32, as the struct holds them."""
    p = dict(DEFAULTS, **overrides)
    return {k: (int(v) if k == "replace_count" else F32(v)) for k, v in p.items()}


def geometry(rows, cols, res, pos):
    """make_geom of csrc/fpe_gridmath.hpp."""
    res = F64(res)
    g = dict(rows=rows, cols=cols, res=res, lenX=F64(rows) * res, lenY=F64(cols) * res, posX=F64(pos[0]), posY=F64(pos[1]))
    g["orgX"], g["orgY"] = F64(0.5) * g["lenX"], F64(0.5) * g["lenY"]
    g["baseX"] = g["posX"] + (g["orgX"] - F64(0.5) * res)
    g["baseY"] = g["posY"] + (g["orgY"] - F64(0.5) * res)
    return g


def within_axis(x, org, pos, length):
    t = -((x - pos) - org)
    return (t >= 0.0) & (t < length)


def index_of(x, org, pos, res):
    return -np.trunc(((x - org) - pos) / res).astype(np.int64)


def cell_pos(base, res, idx):
    return base + res * (-np.asarray(idx)).astype(F64)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def unknown_layers(rows, cols):
    e = np.full((rows, cols), CLEARED, np.uint32).view(F32)
    return e, e.copy()


def set_layers(elev, var):
    """A cell that is NaN in either source becomes unknown in both layers."""
    e, v = bits(elev).copy(), bits(var).copy()
    bad = np.isnan(np.asarray(elev, F32)) | np.isnan(np.asarray(var, F32))
    e[bad] = CLEARED
    v[bad] = CLEARED
    return e.view(F32), v.view(F32)


def move(layer, shift):
    """New cell (i, j) takes old cell (i + sr, j + sc) bit for bit, or the cleared value where that lies outside."""
    old = bits(layer)
    rows, cols = old.shape
    sr, sc = int(shift[0]), int(shift[1])
    new = np.full((rows, cols), CLEARED, np.uint32)
    i0, i1 = max(0, -sr), min(rows, rows - sr)
    j0, j1 = max(0, -sc), min(cols, cols - sc)
    if i0 < i1 and j0 < j1:
        new[i0:i1, j0:j1] = old[i0 + sr:i1 + sr, j0 + sc:j1 + sc]
    return new.view(F32)


def classify(g, p, T, points, roi):
    """Steps 1-6 per point -> (cls, local cell, q): cls 0 non-finite, 1 range, 2 height, 3 off the roi, 4 accepted."""
    pts = np.asarray(points, F32)
    pts = pts.reshape(len(pts), -1)[:, :3] if pts.size else np.zeros((0, 3), F32)
    n = pts.shape[0]
    T = np.asarray(T, F64).reshape(12)
    cls = np.full(n, 4, np.int64)
    cell = np.full(n, -1, np.int64)
    q = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        finite = np.isfinite(pts).all(axis=1)
        xs, ys, zs = (np.where(finite, pts[:, k], F32(0)).astype(F64) for k in range(3))
        r2 = (xs * xs + ys * ys) + zs * zs
        lo, hi = F64(p["min_range"]) * F64(p["min_range"]), F64(p["max_range"]) * F64(p["max_range"])
        in_range = (lo <= r2) & (r2 <= hi)
        xm = ((T[0] * xs + T[1] * ys) + T[2] * zs) + T[3]
        ym = ((T[4] * xs + T[5] * ys) + T[6] * zs) + T[7]
        zm = ((T[8] * xs + T[9] * ys) + T[10] * zs) + T[11]
        in_height = (F64(p["min_z"]) <= zm) & (zm <= F64(p["max_z"]))
        inside = within_axis(xm, g["orgX"], g["posX"], g["lenX"]) & within_axis(ym, g["orgY"], g["posY"], g["lenY"])
        ok = finite & in_range & in_height & inside
        ci = index_of(np.where(ok, xm, g["posX"]), g["orgX"], g["posX"], g["res"]) - roi[0]
        cj = index_of(np.where(ok, ym, g["posY"]), g["orgY"], g["posY"], g["res"]) - roi[1]
        in_roi = ok & (ci >= 0) & (ci < roi[2]) & (cj >= 0) & (cj < roi[3])
        cls[~in_roi] = 3
        cls[~in_height] = 2
        cls[~in_range] = 1
        cls[~finite] = 0  # the earlier test wins: assigned last
        acc = cls == 4
        cell[acc] = ci[acc] * roi[3] + cj[acc]
        q[acc] = np.rint(zm[acc] * 65536.0).astype(np.int64)
    return cls, cell, q


def fuse(elev, var, res, pos, p, T, points, roi):
    """One scan into the layers -> (elevation, variance, info of sixteen int32, per-cell kept counts of the roi, per-cell class:
    0 untouched, 1 new, 2 fused, 3 outlier, 4 replaced)."""
    rows, cols = np.asarray(elev).shape
    g = geometry(rows, cols, res, pos)
    T = np.asarray(T, F64).reshape(12)
    e, v = bits(elev).copy(), bits(var).copy()
    cls, cell, q = classify(g, p, T, points, roi)
    ncell = roi[2] * roi[3]
    acc = cls == 4
    top = np.full(ncell, np.iinfo(np.int64).min, np.int64)
    np.maximum.at(top, cell[acc], q[acc])
    band_q = min(int(np.rint(F64(p["band"]) * 65536.0)), 1 << 31)
    kept = acc.copy()
    kept[acc] = q[acc] >= top[cell[acc]] - band_q
    cnt = np.zeros(ncell, np.int64)
    S = np.zeros(ncell, np.int64)
    np.add.at(cnt, cell[kept], 1)
    np.add.at(S, cell[kept], q[kept])
    cell_cls = np.zeros(ncell, np.int64)
    t = np.nonzero(cnt > 0)[0]
    info = np.zeros(16, np.int32)
    info[0] = len(cls)
    info[1:6] = [(cls == k).sum() for k in range(5)]
    info[6] = int(acc.sum() - kept.sum())
    info[12:] = (0, 0, -1, -1)
    if t.size:
        i, j = roi[0] + t // roi[3], roi[1] + t % roi[3]
        with np.errstate(all="ignore"):
            n32 = cnt[t].astype(F32)
            zm = ((S[t].astype(F64) / cnt[t].astype(F64)) * (1.0 / 65536.0)).astype(F32)
            dx = cell_pos(g["baseX"], g["res"], i) - T[3]
            dy = cell_pos(g["baseY"], g["res"], j) - T[7]
            d2 = (dx * dx + dy * dy).astype(F32)
            vm = np.fmax((p["var_base"] + p["var_range"] * d2) / n32, p["var_min"])
            v_new = np.fmin(vm, p["var_max"])
            hb = e[i, j]
            h, vv = hb.view(F32), v[i, j].view(F32)
            unknown = hb == CLEARED
            d, s = zm - h, vv + vm
            gate2 = p["gate"] * p["gate"]
            outlier = ~unknown & (d * d > gate2 * s)
            replaced = outlier & (p["replace_count"] > 0) & (cnt[t] >= p["replace_count"])
            fused = ~unknown & ~outlier
            k = vv / s
            h_f = h + k * d
            v_f = np.fmin(np.fmax(vv - k * vv, p["var_min"]), p["var_max"])
            v_o = np.fmin(vv + p["var_outlier"], p["var_max"])
            take_new = unknown | replaced
            h2 = np.where(take_new, zm, np.where(fused, h_f, h)).astype(F32)
            v2 = np.where(take_new, v_new, np.where(fused, v_f, v_o)).astype(F32)
        assert all(a.dtype == F32 for a in (n32, zm, d2, vm, v_new, d, s, k, h_f, v_f, v_o, h2, v2)) and np.asarray(gate2).dtype == F32
        ho, vo = h2.view(np.uint32).copy(), v2.view(np.uint32).copy()
        nan = np.isnan(h2) | np.isnan(v2)
        ho[nan] = CLEARED
        vo[nan] = CLEARED
        e[i, j] = ho
        v[i, j] = vo
        cell_cls[t] = np.where(unknown, 1, np.where(fused, 2, np.where(replaced, 4, 3)))
        info[7:12] = [t.size, unknown.sum(), fused.sum(), outlier.sum(), replaced.sum()]
        info[12:] = (i.min(), j.min(), i.max(), j.max())
    return e.view(F32), v.view(F32), info, cnt, cell_cls


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
RES = 0.02
MAPS = {"100x72": (100, 72), "48x40": (48, 40)}


def look_down(cam, yaw=0.0, pitch=0.0):
    """Sensor-to-map transform (3 x 4) of a camera at `cam` looking down (optical axis = map -z), turned by yaw about the map's z and
    tilted by pitch about the sensor's x."""
    down = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    r = rz @ down @ rx
    return np.hstack([r, np.asarray(cam, F64).reshape(3, 1)])


def terrain_height(x, y, centre):
    """A floor with a 0.11 m step along y and a 0.3 m deep hole."""
    z = 0.11 * ((y - centre[1]) > 0.13)
    hole = (np.abs(x - centre[0] + 0.2) < 0.1) & (np.abs(y - centre[1] + 0.2) < 0.1)
    return np.where(hole, -0.3, z)


def pinhole_scan(T, width, height, focal, centre, seed):
    """The points (float32, sensor frame) a width x height pinhole grid sees of terrain_height, with millimetre noise."""
    rng = np.random.default_rng(seed)
    T = np.asarray(T, F64).reshape(3, 4)
    R, cam = T[:, :3], T[:, 3]
    u, v = np.meshgrid(np.arange(width) - 0.5 * (width - 1), np.arange(height) - 0.5 * (height - 1), indexing="xy")
    d = np.stack([u.ravel() / focal, v.ravel() / focal, np.ones(u.size)], axis=1)
    dm = d @ R.T
    t = -cam[2] / dm[:, 2]
    for _ in range(2):  # the plane z = 0 first, then the terrain's height there
        hit = cam + t[:, None] * dm
        t = (terrain_height(hit[:, 0], hit[:, 1], centre) - cam[2]) / dm[:, 2]
    hit = cam + t[:, None] * dm + 0.001 * rng.standard_normal((u.size, 3))
    return ((hit - cam) @ R).astype(F32)


def extras(T, g, cell, n_cluster, centre, seed):
    """A cluster of n_cluster points in one cell (its centre +- a quarter cell, 4 mm above the terrain, heights within a millimetre) and
    points of every drop class: NaN, infinity, too near, too far, too high, off the map — and three that fail two tests at once."""
    rng = np.random.default_rng(seed)
    T = np.asarray(T, F64).reshape(3, 4)
    R, cam = T[:, :3], T[:, 3]
    cx, cy = cell_pos(g["baseX"], g["res"], cell[0]), cell_pos(g["baseY"], g["res"], cell[1])
    m = np.stack([cx + 0.25 * g["res"] * rng.uniform(-1, 1, n_cluster), cy + 0.25 * g["res"] * rng.uniform(-1, 1, n_cluster),
                  terrain_height(cx, cy, centre) + 0.004 + 0.001 * rng.uniform(-1, 1, n_cluster)], axis=1)
    cluster = ((m - cam) @ R).astype(F32)
    far_map = np.array([[g["posX"] + 3.0 * g["lenX"], g["posY"], 0.0], [g["posX"], g["posY"] - 3.0 * g["lenY"], 0.0]])
    high_map = np.array([[g["posX"], g["posY"], 2.5], [g["posX"] + 3.0 * g["lenX"], g["posY"], 2.5]])  # (the second: too high AND off the map)
    bad = np.array([[np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, 0.01], [0.0, 0.0, 50.0], [np.nan, 0.0, 50.0]], F32)
    return np.vstack([cluster, bad, ((far_map - cam) @ R).astype(F32), ((high_map - cam) @ R).astype(F32)])


def prior_layers(rows, cols, centre, pos, seed):
    """A prior that says where every byte came from: each known cell's elevation and variance differ from every other cell's.  Rows in
    the first third are unknown, the middle third agrees with the terrain (fused), the last third lies half a metre off (gated out)."""
    g = geometry(rows, cols, RES, pos)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    k = (i * cols + j).astype(F64)
    z = terrain_height(cell_pos(g["baseX"], g["res"], i), cell_pos(g["baseY"], g["res"], j), centre) + 1e-6 * k
    z = z + 0.5 * (i >= 2 * rows // 3)
    e = z.astype(F32)
    v = (0.0004 + 1e-8 * k).astype(F32)
    e[: rows // 3] = np.nan
    assert np.unique(bits(e)[rows // 3:]).size == (rows - rows // 3) * cols and np.unique(bits(v)).size == rows * cols
    return set_layers(e, v)


def main_case(name="100x72", pos=(0.0, 0.0), seed=1, width=160, height=120, yaw=0.3, pitch=0.0, stride=3, replace_count=24, cam_offset=(0.05, -0.03)):
    """The case most tests share: a pinhole grid in image order (neighbouring points share cells), the extras, a prior of all three
    kinds.  Returns a dict."""
    rows, cols = MAPS[name]
    g = geometry(rows, cols, RES, pos)
    cam = (pos[0] + cam_offset[0], pos[1] + cam_offset[1], 1.2)
    T = look_down(cam, yaw, pitch)
    focal = width * 1.2 / (0.9 * min(g["lenX"], g["lenY"]))  # the image's long axis sees 0.9 of the map's short side from 1.2 m up
    pts = np.vstack([pinhole_scan(T, width, height, focal, pos, seed), extras(T, g, (2 * rows // 3 + 3, cols // 2), 100, pos, seed + 1),
                     extras(T, g, (rows // 2, cols // 3), 90, pos, seed + 2)])
    if stride > 3:
        pts = np.hstack([pts, np.full((len(pts), stride - 3), 7.0, F32)])
    e0, v0 = prior_layers(rows, cols, pos, pos, seed + 4)
    return dict(rows=rows, cols=cols, res=RES, pos=tuple(pos), T=T.reshape(12), points=np.ascontiguousarray(pts), roi=(0, 0, rows, cols),
                params=params(replace_count=replace_count, min_z=-1.0, max_z=2.0), elev=e0, var=v0, stride=stride)


def run(case, points=None, roi=None, elev=None, var=None):
    return fuse(case["elev"] if elev is None else elev, case["var"] if var is None else var, case["res"], case["pos"], case["params"], case["T"],
                case["points"] if points is None else points, case["roi"] if roi is None else roi)


FAR_POS = (1200.0, -41000.0)  # the far-origin tests' magnitudes


def fuse_cases():
    """The cases the GPU test compares against this reference on every byte; tests/test_cpu_scan.py asserts of each that the reference
    alone shows every cell class, every drop class, a cell with more than 64 kept points and a point below the band."""
    return {
        "100x72": main_case("100x72"),
        "48x40": main_case("48x40", seed=11),
        "100x72,stride4": main_case("100x72", seed=21, stride=4),
        # yaw 0.3 rad and pitch 0.7 rad far from the origin: a contracted multiply-add in the transform would change bits here
        "far,pitched": main_case("100x72", pos=FAR_POS, seed=31, pitch=0.7, cam_offset=(0.30, -0.96)),
    }


def shuffled(case, seed):
    return np.ascontiguousarray(case["points"][np.random.default_rng(seed).permutation(len(case["points"]))])


def cell_points(case, cells, per_cell, seed, z=0.05):
    """per_cell points in each of `cells` ((i, j) pairs), within a quarter cell of the centre, heights z +- 2 mm, cell after cell."""
    rng = np.random.default_rng(seed)
    g = geometry(case["rows"], case["cols"], case["res"], case["pos"])
    T = np.asarray(case["T"], F64).reshape(3, 4)
    ij = np.repeat(np.asarray(cells, np.int64).reshape(-1, 2), per_cell, axis=0)
    m = np.stack([cell_pos(g["baseX"], g["res"], ij[:, 0]) + 0.25 * g["res"] * rng.uniform(-1, 1, len(ij)),
                  cell_pos(g["baseY"], g["res"], ij[:, 1]) + 0.25 * g["res"] * rng.uniform(-1, 1, len(ij)), z + 0.002 * rng.uniform(-1, 1, len(ij))], axis=1)
    return np.ascontiguousarray(((m - T[:, 3]) @ T[:, :3]).astype(F32))


def contention_cases(case):
    """4 096 points in one cell, 4 096 along one row of cells, one point per cell of the map."""
    rows, cols = case["rows"], case["cols"]
    return {
        "one cell": cell_points(case, [(rows // 2 + 1, cols // 2 - 1)], 4096, 41),
        "one row": cell_points(case, [(rows // 2, j % cols) for j in range(4096)], 1, 42),
        "one point per cell": cell_points(case, [(i, j) for i in range(rows) for j in range(cols)], 1, 43),
    }


def roi_cases(rows, cols):
    return {"whole map": (0, 0, rows, cols), "one cell": (rows // 2, cols // 3, 1, 1), "ragged corner": (rows - 7, cols - 5, 7, 5)}


def roi_points(case):
    """Points for the roi cases: two in every cell of the map, then the head of the case's own scan."""
    rows, cols = case["rows"], case["cols"]
    return np.ascontiguousarray(np.vstack([cell_points(case, [(i, j) for i in range(rows) for j in range(cols)], 2, 44), case["points"][:5000, :3]]))


TWO_ROIS = ((20, 10, 50, 30), (25, 25, 60, 40))  # two fuses in a row on one state (100 x 72): the second overlaps the first's cells
