"""Plain numpy statement of the scan gap closing (fpe_scan_close*; include/fpe.h, point 5 of the scan block), written from the contract:
an unknown cell between known cells takes a height interpolated along the shortest of the axes that span it, when enough axes span
it and their end heights agree.  The close is a pure function of the elevation layer.  Each search is a loop over the step s with the
layer shifted by s cells; all arithmetic is float32, one numpy operation per rounding.  The terrain is tests/scan_reference.py's.
numpy only; no engine code."""
import numpy as np

from tests import scan_reference as sr

F32, F64 = np.float32, np.float64
CLEARED = sr.CLEARED
DEFAULTS = dict(reach=4, max_gap=5, min_axes=2, max_spread=0.08)
AXES = ((0, 1), (1, 0), (1, 1), (1, -1))  # (row, column) steps
KNOWN, FILLED, NO_SUPPORT, REJECTED_AXES, REJECTED_SPREAD = range(5)
INFO_FIELDS = ("cells", "known", "unknown", "filled", "no_support", "rejected_axes", "rejected_spread", "reserved")
INFO_DTYPE = np.dtype([(k, "<i4") for k in INFO_FIELDS] + [("bbox", "<i4", (4,)), ("reserved2", "<i4", (4,))])
assert INFO_DTYPE.itemsize == 64


def params(**overrides):
    """The defaults of fpe_scan_close_params_defaults with any field replaced; max_spread as float32, as the struct holds it."""
    p = dict(DEFAULTS, **overrides)
    return {k: (F32(v) if k == "max_spread" else int(v)) for k, v in p.items()}


def shifted(a, dr, dc, fill):
    """b[i, j] = a[i + dr, j + dc], and `fill` where that lies off the map."""
    rows, cols = a.shape
    b = np.full_like(a, fill)
    i0, i1 = max(0, -dr), min(rows, rows - dr)
    j0, j1 = max(0, -dc), min(cols, cols - dc)
    if i0 < i1 and j0 < j1:
        b[i0:i1, j0:j1] = a[i0 + dr:i1 + dr, j0 + dc:j1 + dc]
    return b


def first_known(e, dr, dc, reach):
    """Per cell c: the least s in 1..reach for which c + s (dr, dc) is known (0: none; off the map is unknown), and the height there."""
    known = ~np.isnan(e)
    s_out = np.zeros(e.shape, np.int64)
    h_out = np.full(e.shape, np.nan, F32)
    for s in range(1, reach + 1):
        take = (s_out == 0) & shifted(known, s * dr, s * dc, False)
        s_out[take] = s
        h_out[take] = shifted(e, s * dr, s * dc, F32(np.nan))[take]
    return s_out, h_out


def close_whole(elev, kp=None):
    """The rule for every cell of the layer -> (closed layer, class per cell as uint8)."""
    kp = params() if kp is None else kp
    e = np.ascontiguousarray(elev, F32)
    known = ~np.isnan(e)
    n = np.zeros(e.shape, np.int64)
    lo, hi = np.full(e.shape, np.inf, F32), np.full(e.shape, -np.inf, F32)
    best = np.full(e.shape, 1 << 30, np.int64)  # s+ + s- of the chosen axis
    v = np.full(e.shape, np.nan, F32)
    with np.errstate(all="ignore"):
        for dr, dc in AXES:
            sp, hp = first_known(e, dr, dc, kp["reach"])
            sm, hm = first_known(e, -dr, -dc, kp["reach"])
            spans = (sp > 0) & (sm > 0) & (sp + sm - 1 <= kp["max_gap"])
            n += spans
            lo = np.where(spans, np.minimum(lo, np.minimum(hp, hm)), lo)
            hi = np.where(spans, np.maximum(hi, np.maximum(hp, hm)), hi)
            va = hm + (hp - hm) * (sm.astype(F32) / (sp + sm).astype(F32))
            assert va.dtype == F32
            better = spans & (sp + sm < best)  # (strictly: the lowest axis number among equals)
            v = np.where(better, va, v)
            best = np.where(better, sp + sm, best)
        agree = (hi - lo) <= kp["max_spread"]  # (a NaN difference, of inf - inf, does not agree)
    cls = np.full(e.shape, FILLED, np.uint8)
    cls[np.isnan(v)] = REJECTED_SPREAD
    cls[~agree] = REJECTED_SPREAD
    cls[n < kp["min_axes"]] = REJECTED_AXES
    cls[n == 0] = NO_SUPPORT
    cls[known] = KNOWN  # the earlier step wins: assigned last
    out = np.full(e.shape, CLEARED, np.uint32)
    out[known] = sr.bits(e)[known]
    out[cls == FILLED] = sr.bits(v)[cls == FILLED]
    return out.view(F32), cls


def close(elev, kp=None, rect=None):
    """fpe_scan_close of `rect` (row0, col0, n_rows, n_cols; None: the whole layer) -> (closed rectangle, classes, info record)."""
    rows, cols = np.asarray(elev).shape
    r0, c0, nr, nc = (0, 0, rows, cols) if rect is None else rect
    out, cls = close_whole(elev, kp)
    out, cls = np.ascontiguousarray(out[r0:r0 + nr, c0:c0 + nc]), np.ascontiguousarray(cls[r0:r0 + nr, c0:c0 + nc])
    info = np.zeros(1, INFO_DTYPE)[0]
    info["cells"] = nr * nc
    for k, name in enumerate(("known", "filled", "no_support", "rejected_axes", "rejected_spread")):
        info[name] = int((cls == k).sum())
    info["unknown"] = info["cells"] - info["known"]
    ii, jj = np.nonzero(cls == FILLED)
    info["bbox"] = (r0 + ii.min(), c0 + jj.min(), r0 + ii.max(), c0 + jj.max()) if ii.size else (0, 0, -1, -1)
    return out, cls, info


def words(info):
    return np.frombuffer(np.asarray(info).tobytes(), np.int32)


def ingest_rects(rows, cols, roi, shift, reach):
    """The rectangles fpe_scan_ingest_closed closes, in the order of its patches: the roi grown by `reach`, then the strip of rows and
    the strip of columns whose neighbours a move took off the map."""
    r0, c0 = max(0, roi[0] - reach), max(0, roi[1] - reach)
    r1, c1 = min(rows, roi[0] + roi[2] + reach), min(cols, roi[1] + roi[3] + reach)
    rects = [(r0, c0, r1 - r0, c1 - c0)]
    sr_, sc_ = int(shift[0]), int(shift[1])
    if sr_ != 0:
        rects.append((0 if sr_ > 0 else rows - reach, 0, reach, cols))
    if sc_ != 0:
        rects.append((0, 0 if sc_ > 0 else cols - reach, rows, reach))
    return rects


# ---- the states ----------------------------------------------------------------------------------------------------------------------
SPECIALS = ((5, 20, np.inf), (8, 30, -np.inf), (11, 24, -0.0))  # (row, column, height): each with unknown neighbours


def holey(rows, cols, seed=1, pos=(0.0, 0.0)):
    """A known layer on scan_reference's terrain (every cell's height its own, a +0.5 m step at two thirds of the rows) with holes of
    every kind: 30 % of the cells at random, every seventh row, a band of three rows and one of seven (wider than any max_gap), a
    two-column gap over the columns 63-64 and a two-row gap over the rows 15-16 (the tiled form's seams), every other cell of the two
    rows at the step's edge, and three cells of +inf, -inf and -0.0 between unknown neighbours."""
    rng = np.random.default_rng(seed)
    g = sr.geometry(rows, cols, sr.RES, pos)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    k = (i * cols + j).astype(F64)
    z = sr.terrain_height(sr.cell_pos(g["baseX"], g["res"], i), sr.cell_pos(g["baseY"], g["res"], j), pos) + 1e-6 * k
    step = 2 * rows // 3
    e = (z + 0.5 * (i >= step)).astype(F32)
    e[rng.random((rows, cols)) < 0.3] = np.nan
    e[6::7] = np.nan
    e[22:25] = np.nan
    e[rows // 2 - 12:rows // 2 - 5] = np.nan
    e[15:17] = np.nan
    e[:, 63:65] = np.nan
    e[step - 1, 0::2] = np.nan
    e[step, 1::2] = np.nan
    for r, c, h in SPECIALS:
        e[r, c - 1:c + 2] = np.nan
        e[r, c] = h
    return e


def holey_layers(rows, cols, seed=1, pos=(0.0, 0.0)):
    """holey as a state's two layers (a variance that is unknown where the elevation is)."""
    return sr.set_layers(holey(rows, cols, seed, pos), np.full((rows, cols), 0.0004, F32))


# ---- a sequence of ingests (the CPU and the GPU tests share it) -------------------------------------------------------------------------
# (shift, roi, with the clear) on a 100 x 72 state: every sign of sr and sc, a roi in each of two corners, one |shift| >= the size
INGEST_STEPS = (
    ((0, 0), (20, 10, 50, 30), False),
    ((3, -2), (25, 25, 60, 40), True),
    ((-4, 5), (0, 0, 30, 20), False),
    ((0, 7), (70, 50, 30, 22), True),
    ((2, -100), (10, 5, 60, 50), False),
    ((-5, 0), (20, 10, 50, 30), True),
)


def ingest_state(elev, var, case, step, clear_params=None):
    """What move, clear (when the step says so) and fuse of the case's points leave of a state's layers; the position stays the case's."""
    from tests import scan_clear_reference as cr
    shift, roi, with_clear = step
    e, v = sr.move(elev, shift), sr.move(var, shift)
    if with_clear:
        e, v = cr.run(case, cp=clear_params, roi=roi, elev=e, var=v)[:2]
    return sr.run(case, roi=roi, elev=e, var=v)[:2]


def patched(snapshot, state_elev, shift, rects, kp=None):
    """The snapshot's elevation after an ingest: shifted, then the closed rectangles of the new state written over it in order."""
    out = sr.bits(sr.move(snapshot, shift)).copy()
    for r0, c0, nr, nc in rects:
        out[r0:r0 + nr, c0:c0 + nc] = sr.bits(close(state_elev, kp, (r0, c0, nr, nc))[0])
    return out.view(F32)
