"""Plain numpy statement of the elevation-driven map update (fpe_update_elevation*, include/fpe.h), written from the contract: the
reach R, the sets C and B, the dirty set D, the composed elevation E*, the position that keeps the carried cells' centres where
they were, and the cases the CPU and the GPU tests share.  Reuses tests/map_update_reference.py.  numpy only."""
import numpy as np

from tests import map_update_reference as mu

DEFAULT_RADII = dict(normal_radius=0.05, roughness_radius=0.05, step_first_radius=0.08, step_second_radius=0.08)


def halo(radius, res):
    """filter_halo of csrc/fpe_filters.hpp: int(r / res) + 1 in double arithmetic."""
    return int(float(radius) / float(res)) + 1


def reach(res, normal_radius=0.05, roughness_radius=0.05, step_first_radius=0.08, step_second_radius=0.08):
    """R = max(hN, hR, h1 + h2)."""
    return max(halo(normal_radius, res), halo(roughness_radius, res), halo(step_first_radius, res) + halo(step_second_radius, res))


def dilate(mask, R):
    """Cells within Chebyshev distance R of a cell of `mask`, clipped to the map."""
    rows, cols = mask.shape
    out = np.zeros_like(mask)
    ii, jj = np.nonzero(mask)
    for i, j in zip(ii, jj):
        out[max(0, i - R):min(rows, i + R + 1), max(0, j - R):min(cols, j + R + 1)] = True
    return out


def changed_set(rows, cols, shift, rects):
    """C: the cells of every patch rectangle, and every cell without a source."""
    c = ~mu.carried_mask(rows, cols, shift)
    for row0, col0, nr, nc in rects:
        c[row0:row0 + nr, col0:col0 + nc] = True
    return c


def clipped_set(rows, cols, shift, R):
    """B: lines whose window the map edge clips differently before and after the move (the carried cells among them)."""
    sr, sc = int(shift[0]), int(shift[1])
    b = np.zeros((rows, cols), bool)
    if sr != 0:
        i = np.arange(rows)
        b[(i < R) | (i >= rows - R) | (i + sr < R) | (i + sr >= rows - R), :] = True
    if sc != 0:
        j = np.arange(cols)
        b[:, (j < R) | (j >= cols - R) | (j + sc < R) | (j + sc >= cols - R)] = True
    return b


def dirty_set(rows, cols, shift, rects, R):
    """D = {cells within Chebyshev distance R of a cell of C} united with B, clipped to the map."""
    c = changed_set(rows, cols, shift, rects)
    if c.all():
        return c
    # (dilating a few rectangles cell by cell is slow: the bands without a source are whole lines, the rest are rectangles)
    d = np.zeros((rows, cols), bool)
    lines_r, lines_c = np.nonzero(c.all(axis=1))[0], np.nonzero(c.all(axis=0))[0]
    for i in lines_r:
        d[max(0, i - R):min(rows, i + R + 1), :] = True
    for j in lines_c:
        d[:, max(0, j - R):min(cols, j + R + 1)] = True
    for row0, col0, nr, nc in rects:
        d[max(0, row0 - R):min(rows, row0 + nr + R), max(0, col0 - R):min(cols, col0 + nc + R)] = True
    return d | clipped_set(rows, cols, shift, R)


def compose_elevation(elev, shift, patches):
    """E*: fpe_update_map's steps 1-3 on the elevation layer.  patches: [(row0, col0, values), ...]."""
    elev = np.asarray(elev, np.float32)
    rows, cols = elev.shape
    sr, sc = int(shift[0]), int(shift[1])
    new = np.full((rows, cols), mu.CLEARED, np.uint32)
    m = mu.carried_mask(rows, cols, shift)
    ii, jj = np.nonzero(m)
    new[ii, jj] = elev.view(np.uint32)[ii + sr, jj + sc]
    for row0, col0, pe in patches:
        pe = np.asarray(pe, np.float32)
        new[row0:row0 + pe.shape[0], col0:col0 + pe.shape[1]] = pe.view(np.uint32)
    return new.view(np.float32)


def shifted(layer, shift):
    """The base's value at (i + sr, j + sc) for every carried cell, the cleared value elsewhere (bit patterns kept)."""
    return compose_elevation(layer, shift, [])


def moved_position(position, shift, res):
    """getPosition() of the map after a move by `shift` cells: cell (i, j) of the new map lies where cell (i + sr, j + sc) of the
    old one lay (a cell's centre is position + origin - index * resolution on either axis)."""
    return (float(position[0]) - int(shift[0]) * float(res), float(position[1]) - int(shift[1]) * float(res))


def grown_rect_cells(rows, cols, rects, grow):
    """Cells of the union of `rects` ((r0, c0, r1, c1), half-open), each grown by `grow` per side and clipped."""
    m = np.zeros((rows, cols), bool)
    for r0, c0, r1, c1 in rects:
        m[max(0, r0 - grow):min(rows, r1 + grow), max(0, c0 - grow):min(cols, c1 + grow)] = True
    return int(m.sum())


def dirty_rects(rows, cols, shift, rects, R):
    """D as rectangles (r0, c0, r1, c1): runs of whole dirty rows, runs of whole dirty columns, the grown patch rectangles."""
    d = dirty_set(rows, cols, shift, [], R)
    out = []
    for axis, n in ((1, rows), (0, cols)):
        full = d.all(axis=axis)
        k = 0
        while k < n:
            if not full[k]:
                k += 1
                continue
            e = k
            while e < n and full[e]:
                e += 1
            out.append((k, 0, e, cols) if axis == 1 else (0, k, rows, e))
            k = e
    for row0, col0, nr, nc in rects:
        out.append((max(0, row0 - R), max(0, col0 - R), min(rows, row0 + nr + R), min(cols, col0 + nc + R)))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
MAPS = [(100, 72, 0.02), (48, 40, 0.02), (160, 96, 0.01)]
PATCH_SETS = mu.PATCH_SETS + ("corner00", "tilecorner")


def shifts(rows, cols):
    return [(0, 0), (5, 3), (-7, 0), (0, -2), (rows, 0), (-3, cols + 1)]


def patch_rects(name, rows, cols, shift):
    """mu.patch_set_rects, a 1 x 1 patch at the map's first corner, and a patch straddling the corner of a 32 x 16 tile."""
    if name == "corner00":
        return [(0, 0, 1, 1)]
    if name == "tilecorner":
        return [(30, 14, 4, 4)]  # rows 30 .. 33, columns 14 .. 17: four tiles of 32 x 16 (and of 32 x 32 / 16 x 16 in rows)
    if name == "interior" and not mu.carried_mask(rows, cols, shift).any():
        return [(rows // 3, cols // 3, max(1, rows // 3), max(1, cols // 2))]
    return mu.patch_set_rects(name, rows, cols, shift)


def cases():
    for rows, cols, res in MAPS:
        for shift in shifts(rows, cols):
            for name in PATCH_SETS:
                yield rows, cols, res, shift, name


def terrain(rows, cols, seed, holes=0.02):
    """Seeded rough terrain with NaN holes: smooth hills, a riser, noise."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    z = 0.08 * np.sin(i / 9.0 + rng.uniform(0, 6)) * np.cos(j / 7.0 + rng.uniform(0, 6)) + 0.004 * rng.standard_normal((rows, cols))
    z += 0.11 * (j > cols * rng.uniform(0.3, 0.7))
    z = z.astype(np.float32)
    z[rng.random((rows, cols)) < holes] = np.nan
    return z


def patch_values(rects, seed):
    """Fresh elevation values for every rectangle (some holes among them)."""
    rng = np.random.default_rng(seed)
    out = []
    for row0, col0, nr, nc in rects:
        v = (0.05 * rng.standard_normal((nr, nc)) + 0.02).astype(np.float32)
        v[rng.random((nr, nc)) < 0.03] = np.nan
        out.append((row0, col0, v))
    return out
