"""Plain numpy statement of the scan visibility clearing (fpe_scan_clear*; include/fpe.h, point 4 of the scan block), written from the
contract: every ray from the sensor's origin to a point that passes the fuse's tests 1-4 is sampled by a fixed rule in f64, a sample
that passes more than `margin` below a known cell's height counts against that cell once per ray, and a cell with `min_hits` such rays
becomes unknown in both layers.  All samples of a scan are laid out in one array (np.repeat over the rays, a per-ray arange), and "once
per ray and cell" is a np.unique over (ray, cell).  Geometry, classification and cases are tests/scan_reference.py's.  numpy only."""
import numpy as np

from tests import scan_reference as sr

F32, F64 = np.float32, np.float64
CLEARED = sr.CLEARED
DEFAULTS = dict(sample_step=0.5, margin=0.10, start_samples=2, end_samples=4, min_hits=2, ray_stride=1, max_samples=4096, reserved=0)
FLOAT_FIELDS = ("sample_step", "margin")
INFO_DTYPE = np.dtype([("n_points", "<i4"), ("strided_out", "<i4"), ("dropped_points", "<i4"), ("rays", "<i4"), ("rays_long", "<i4"),
                       ("rays_empty", "<i4"), ("cells_hit", "<i4"), ("cells_cleared", "<i4"), ("bbox", "<i4", (4,)), ("samples_in_roi", "<i8"),
                       ("hit_pairs", "<i8")])
assert INFO_DTYPE.itemsize == 64


def params(**overrides):
    """The defaults of fpe_scan_clear_params_defaults with any field replaced; floats as float32, as the struct holds them."""
    p = dict(DEFAULTS, **overrides)
    return {k: (F32(v) if k in FLOAT_FIELDS else int(v)) for k, v in p.items()}


def words(info):
    """An info record as its sixteen int32 words."""
    return np.frombuffer(np.asarray(info).tobytes(), np.int32)


def flat(info):
    """An info record as fourteen integers: the eight counters, the bbox, samples_in_roi, hit_pairs."""
    return [int(info[k]) for k in INFO_DTYPE.names[:8]] + [int(b) for b in info["bbox"]] + [int(info["samples_in_roi"]), int(info["hit_pairs"])]


def samples(g, p, cp, T, points, roi):
    """Steps 1-6 -> (counters, ray of each sample, local cell of each sample or -1, z of each sample); the counters are a dict of the
    per-point info fields.  Rays are numbered in the order of their points."""
    pts = np.asarray(points, F32)
    pts = pts.reshape(len(pts), -1)[:, :3] if pts.size else np.zeros((0, 3), F32)
    n = len(pts)
    T = np.asarray(T, F64).reshape(12)
    sel = np.arange(n) % cp["ray_stride"] == 0
    pts = pts[sel]  # the others are not read
    cls = sr.classify(g, p, T, pts, roi)[0]
    ray = cls >= 3  # tests 1-4 passed; where the end lies does not matter
    with np.errstate(all="ignore"):
        xs, ys, zs = (pts[ray, k].astype(F64) for k in range(3))
        xm = ((T[0] * xs + T[1] * ys) + T[2] * zs) + T[3]
        ym = ((T[4] * xs + T[5] * ys) + T[6] * zs) + T[7]
        zm = ((T[8] * xs + T[9] * ys) + T[10] * zs) + T[11]
        dx, dy, dz = xm - T[3], ym - T[7], zm - T[11]
        m = np.fmax(np.fabs(dx), np.fabs(dy))
        step = F64(cp["sample_step"]) * g["res"]
        Kd = np.ceil(m / step)
    long_ = ~(Kd <= F64(cp["max_samples"]))  # compared in f64, before any conversion (a NaN, of an overflowed transform, is long too)
    K = np.where(long_, 0, Kd).astype(np.int64)
    k0, k1 = cp["start_samples"], K - cp["end_samples"]
    cnt = np.where(long_, 0, np.maximum(k1 - k0, 0))
    counters = dict(n_points=n, strided_out=int(n - sel.sum()), dropped_points=int((~ray).sum()), rays=int(ray.sum()), rays_long=int(long_.sum()),
                    rays_empty=int((~long_ & (cnt == 0)).sum()))
    total = int(cnt.sum())
    rid = np.repeat(np.arange(len(cnt)), cnt)
    k = k0 + (np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    t = k.astype(F64) / K[rid].astype(F64)
    x = T[3] + t * dx[rid]
    y = T[7] + t * dy[rid]
    z = T[11] + t * dz[rid]
    inside = sr.within_axis(x, g["orgX"], g["posX"], g["lenX"]) & sr.within_axis(y, g["orgY"], g["posY"], g["lenY"])
    ci = sr.index_of(np.where(inside, x, g["posX"]), g["orgX"], g["posX"], g["res"]) - roi[0]
    cj = sr.index_of(np.where(inside, y, g["posY"]), g["orgY"], g["posY"], g["res"]) - roi[1]
    inside &= (ci >= 0) & (ci < roi[2]) & (cj >= 0) & (cj < roi[3])
    cell = np.where(inside, ci * roi[3] + cj, -1)
    return counters, rid, cell, z, cnt


def clear(elev, var, res, pos, p, cp, T, points, roi):
    """One scan's rays against the layers -> (elevation, variance, info record, per-cell hits of the roi)."""
    rows, cols = np.asarray(elev).shape
    g = sr.geometry(rows, cols, res, pos)
    e, v = sr.bits(elev).copy(), sr.bits(var).copy()
    counters, rid, cell, z, _ = samples(g, p, cp, T, points, roi)
    ncell = roi[2] * roi[3]
    ins = cell >= 0
    rid, cell, z = rid[ins], cell[ins], z[ins]
    i, j = roi[0] + cell // roi[3], roi[1] + cell % roi[3]
    h = e[i, j].view(F32)
    viol = ~np.isnan(h) & ((z + F64(cp["margin"])) < h.astype(F64))
    pairs = np.unique(rid[viol] * ncell + cell[viol])  # a ray counts against a cell once
    hits = np.bincount(pairs % ncell, minlength=ncell)
    gone = np.nonzero(hits >= cp["min_hits"])[0]
    gi, gj = roi[0] + gone // roi[3], roi[1] + gone % roi[3]
    e[gi, gj] = CLEARED
    v[gi, gj] = CLEARED
    info = np.zeros(1, INFO_DTYPE)[0]
    for name, val in counters.items():
        info[name] = val
    info["cells_hit"], info["cells_cleared"] = int((hits >= 1).sum()), gone.size
    info["bbox"] = (gi.min(), gj.min(), gi.max(), gj.max()) if gone.size else (0, 0, -1, -1)
    info["samples_in_roi"], info["hit_pairs"] = int(ins.sum()), pairs.size
    return e.view(F32), v.view(F32), info, hits


def run(case, cp=None, points=None, roi=None, elev=None, var=None):
    return clear(case["elev"] if elev is None else elev, case["var"] if var is None else var, case["res"], case["pos"], case["params"],
                 params() if cp is None else cp, case["T"], case["points"] if points is None else points, case["roi"] if roi is None else roi)


# ---- the states ----------------------------------------------------------------------------------------------------------------------
def own_state(case):
    """What a fuse of the case's own points into unknown layers leaves: the state a sensor that saw only this scan holds."""
    e0, v0 = sr.unknown_layers(case["rows"], case["cols"])
    return sr.run(case, elev=e0, var=v0)[:2]


def ghost_box(case):
    rows, cols = case["rows"], case["cols"]
    return rows // 2 - 10, cols // 2 + 5, 6, 6


def ghost_state(case):
    """own_state with a 6 x 6 box 0.4 m higher (unknown cells of it: 0.4 m, variance 0.001): something that stood there and left."""
    e, v = (a.copy() for a in own_state(case))
    r0, c0, nr, nc = ghost_box(case)
    be, bv = e[r0:r0 + nr, c0:c0 + nc], v[r0:r0 + nr, c0:c0 + nc]
    unknown = np.isnan(be)
    be[~unknown] += F32(0.4)
    be[unknown] = F32(0.4)
    bv[unknown] = F32(0.001)
    return e, v


def raised(case):
    """The case's prior with every known cell two metres up: above the sensor, so every sample over a known cell violates it."""
    e = case["elev"].copy()
    e[~np.isnan(e)] += F32(2.0)
    return sr.set_layers(e, case["var"])


# The contention cases' points lie almost under the sensor: a tenth of a cell per sample and no skipped ends give their rays samples
CONTENTION = dict(sample_step=0.1, start_samples=0, end_samples=0)

# A case in which every per-point counter is above zero: every third point casts a ray, and rays of more than 90 samples are not walked
EVERY_COUNTER = dict(ray_stride=3, max_samples=60)


def grazing_points(case, n=64):
    """Rays that end just beyond the map's far side at floor height: from 1.2 m up they come down over the last rows (where the cases' own
    prior stands half a metre high), have more than a hundred samples each, and none ends in a roi."""
    g = sr.geometry(case["rows"], case["cols"], case["res"], case["pos"])
    T = np.asarray(case["T"], F64).reshape(3, 4)
    y = g["posY"] + 0.4 * g["lenY"] * np.linspace(-1.0, 1.0, n)
    m = np.stack([np.full(n, g["posX"] - 0.55 * g["lenX"]), y, np.zeros(n)], axis=1)
    return np.ascontiguousarray(((m - T[:, 3]) @ T[:, :3]).astype(F32))
