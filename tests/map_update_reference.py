"""Plain numpy reference of the incremental map update (fpe_update_map*, include/fpe.h), written from the contract: the base's
canonical layers shifted by whole cells, grid_map's cleared value where nothing is carried, the patches written over that in
order.  Also the three forms a patch source can take, the shifts and patch sets of tests/test_gpu_map_update.py, and the circular
buffer's side of the shift convention.  numpy only."""
import numpy as np

CLEARED = np.uint32(0x7FC00000)  # the quiet NaN of a cell grid_map::move has cleared
FORMS = ("packed", "pitched", "colmajor")


def compose(trav, elev, shift, patches):
    """(trav', elev') of the contract.  patches: [(row0, col0, trav values, elev values), ...] with 2-D arrays of any strides."""
    trav, elev = np.asarray(trav, np.float32), np.asarray(elev, np.float32)
    rows, cols = trav.shape
    sr, sc = int(shift[0]), int(shift[1])
    out = []
    for base in (trav, elev):
        bits = base.view(np.uint32)
        new = np.empty((rows, cols), np.uint32)
        for i in range(rows):
            for j in range(cols):
                si, sj = i + sr, j + sc
                new[i, j] = bits[si, sj] if 0 <= si < rows and 0 <= sj < cols else CLEARED
        out.append(new)
    for row0, col0, pt, pe in patches:
        pt, pe = np.asarray(pt), np.asarray(pe)
        assert pt.dtype == np.float32 and pe.dtype == np.float32 and pt.shape == pe.shape and pt.ndim == 2
        nr, nc = pt.shape
        assert nr > 0 and nc > 0 and row0 >= 0 and col0 >= 0 and row0 + nr <= rows and col0 + nc <= cols
        for new, p in zip(out, (pt, pe)):
            for r in range(nr):
                for c in range(nc):
                    new[row0 + r, col0 + c] = p[r, c:c + 1].view(np.uint32)[0]
    return out[0].view(np.float32), out[1].view(np.float32)


def carried_mask(rows, cols, shift):
    """Cells of the new map that take a value of the base."""
    ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    si, sj = ii + int(shift[0]), jj + int(shift[1])
    return (si >= 0) & (si < rows) & (sj >= 0) & (sj < cols)


# ---- patch sources ---------------------------------------------------------------------------------------------------------------
def patch_source(values, form, rows, cols, row0, col0, fill=np.float32(-77.0)):
    """`values` ((n_rows, n_cols) f32) as a patch source of one of the three forms; element (r, c) of the result is values[r, c].
    packed: a C-contiguous array of its own.  pitched: a view into a wider row-major array (pitch n_cols + 3).  colmajor: a view
    into the flat column-major message buffer of a rows x cols map with start index (0, 0) (buffer cell (bi, bj) at bj * rows +
    bi) at the rectangle's place — a non-wrapping region of the message, which is what grid_map::move hands out."""
    values = np.asarray(values, np.float32)
    nr, nc = values.shape
    if form == "packed":
        out = np.ascontiguousarray(values).copy()
    elif form == "pitched":
        wide = np.full((nr + 1, nc + 3), fill, np.float32)
        out = wide[:nr, 2:2 + nc]
        out[...] = values
        assert out.strides == (4 * (nc + 3), 4)
    elif form == "colmajor":
        flat = np.full(rows * cols, fill, np.float32)
        out = flat.reshape(cols, rows).T[row0:row0 + nr, col0:col0 + nc]
        out[...] = values
        assert out.strides == (4, 4 * rows) and np.shares_memory(out, flat)
    else:
        raise ValueError(form)
    assert np.array_equal(out.view(np.uint32), values.view(np.uint32))
    return out


# ---- the circular buffer's side of the shift ---------------------------------------------------------------------------------------
def move_buffer(buf, rows, cols, start, shift, order):
    """What grid_map::move does to a message buffer (`buf` of ingest_reference.message_buffer, start index `start`) for the index
    shift `shift`: the buffer rows / columns that held the cells falling out of the map are cleared (they are the new map's
    leading edge), nothing else is touched, and the start index advances by the shift, wrapped.  Returns (buffer, new start)."""
    b = np.array(buf, np.float32).reshape(-1).copy().view(np.uint32)
    grid = b.reshape(rows, cols) if order == "row" else b.reshape(cols, rows).T  # grid[bi, bj]
    for axis, (size, s, d) in enumerate(((rows, start[0], int(shift[0])), (cols, start[1], int(shift[1])))):
        if abs(d) >= size:
            lines = range(size)
        elif d >= 0:
            lines = [(s + k) % size for k in range(d)]  # the oldest lines at the start become the newest at the end
        else:
            lines = [(s - k) % size for k in range(1, -d + 1)]
        for ln in lines:
            if axis == 0:
                grid[ln, :] = CLEARED
            else:
                grid[:, ln] = CLEARED
    new_start = ((start[0] + int(shift[0])) % rows, (start[1] + int(shift[1])) % cols)
    out = b.view(np.float32)
    return (out.reshape(rows, cols) if order == "row" else out), new_start


# ---- the cases of tests/test_gpu_map_update.py --------------------------------------------------------------------------------------
FULL_SHAPES = [(65, 63), (129, 96), (127, 100)]
SMALL_SHAPES = [(7, 31), (1, 70), (70, 1)]
PATCH_SHIFT = (5, -37)  # the shift the patch sets are run with


def shifts(rows, cols):
    """(0, 0); one cell each way; around the 32-column word (misaligned source rows); around the 8-row group with its + 1 offset;
    a mixed one; one cell carried; nothing carried."""
    out = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]
    out += [(0, s * k) for k in (31, 32, 33) for s in (1, -1)]
    out += [(s * k, 0) for k in (7, 8, 9) for s in (1, -1)]
    out += [(5, -37), (rows - 1, -(cols - 1)), (rows, 0), (-rows - 5, cols + 3)]
    return out


def band_rects(rows, cols, shift):
    """The rectangles no cell of the base is carried into (grid_map::move's new regions), disjoint: the row band over the full
    width, the column band over the remaining rows."""
    sr, sc = int(shift[0]), int(shift[1])
    if abs(sr) >= rows or abs(sc) >= cols:
        return [(0, 0, rows, cols)]
    out = []
    r_lo, r_hi = (0, rows - sr) if sr >= 0 else (-sr, rows)  # carried rows
    if sr > 0:
        out.append((rows - sr, 0, sr, cols))
    elif sr < 0:
        out.append((0, 0, -sr, cols))
    if sc > 0:
        out.append((r_lo, cols - sc, r_hi - r_lo, sc))
    elif sc < 0:
        out.append((r_lo, 0, r_hi - r_lo, -sc))
    return out


def patch_set_rects(name, rows, cols, shift):
    """[(row0, col0, n_rows, n_cols), ...] of a named patch set."""
    nw = (cols + 31) // 32
    if name == "none":
        return []
    if name == "bands":
        return band_rects(rows, cols, shift)
    if name == "interior":  # inside the carried cells
        m = carried_mask(rows, cols, shift)
        ii, jj = np.nonzero(m)
        r0, r1, c0, c1 = ii.min(), ii.max() + 1, jj.min(), jj.max() + 1
        nr, nc = max(1, (r1 - r0) // 3), max(1, (c1 - c0) // 2)
        return [(int(r0 + (r1 - r0 - nr) // 2), int(c0 + (c1 - c0 - nc) // 2), int(nr), int(nc))]
    if name == "overlap":
        a = (rows // 5, cols // 4, max(2, rows // 3), max(2, cols // 3))
        return [a, (a[0] + a[2] // 2, a[1] + a[3] // 3, min(a[2], rows - a[0] - a[2] // 2), min(a[3], cols - a[1] - a[3] // 3))]
    if name == "corner":
        return [(rows - 1, cols - 1, 1, 1)]
    if name == "lastword":  # the last plane word and the last 8-row group (row i lies in group (i + 1) >> 3), entered from outside both
        row0, col0 = max(0, 8 * (rows >> 3) - 1 - 3), max(0, 32 * (nw - 1) - 5)
        return [(row0, col0, rows - row0, cols - col0)]
    if name == "whole":
        return [(0, 0, rows, cols)]
    if name == "eight":
        out = []
        for k in range(8):
            nr, nc = 1 + (rows * (k + 2)) // 23 % max(1, rows // 2), 1 + (cols * (k + 3)) // 19 % max(1, cols // 2)
            out.append(((k * 37) % (rows - nr + 1), (k * 53) % (cols - nc + 1), nr, nc))
        return out
    raise ValueError(name)


PATCH_SETS = ("none", "bands", "interior", "overlap", "corner", "lastword", "whole", "eight")


def plane_class(trav, pair):
    """The D / Df / C / F bits of every cell for a threshold pair, as one small integer (the planes' predicates)."""
    v = np.asarray(trav, np.float32)
    fin = np.isfinite(v)
    with np.errstate(invalid="ignore"):
        d, c = v < np.float32(pair[0]), v < np.float32(pair[1])
    return d.astype(np.uint8) | ((d & fin).astype(np.uint8) << 1) | ((c & fin).astype(np.uint8) << 2) | (fin.astype(np.uint8) << 3)
