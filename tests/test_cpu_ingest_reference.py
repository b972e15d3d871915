"""The numpy reference of the map ingest (tests/ingest_reference.py) pinned on its own: hand-written message buffers, the round
trip through the independently written inverse, and — for every shape and start index tests/test_gpu_ingest.py uses — every
hostile category at every place, read back from the arrays."""
import numpy as np
import pytest

from tests import ingest_reference as ir

# canonical 3 x 4 layer: cell (i, j) holds 10 * i + j
CANON = np.array([[0, 1, 2, 3], [10, 11, 12, 13], [20, 21, 22, 23]], np.float32)

HAND = [
    # start (0, 0), column-major: the columns one after the other
    ((0, 0), "col", [0, 10, 20, 1, 11, 21, 2, 12, 22, 3, 13, 23]),
    # start (1, 0), row-major: canonical row 0 sits in buffer row 1, the last canonical row has wrapped into buffer row 0
    ((1, 0), "row", [[20, 21, 22, 23], [0, 1, 2, 3], [10, 11, 12, 13]]),
    # start (2, 3), row-major: canonical (0, 0) sits in buffer cell (2, 3); buffer row 0 holds canonical row 1, buffer column 0
    # canonical column 1
    ((2, 3), "row", [[11, 12, 13, 10], [21, 22, 23, 20], [1, 2, 3, 0]]),
    # the same start index, column-major: that buffer column by column
    ((2, 3), "col", [11, 21, 1, 12, 22, 2, 13, 23, 3, 10, 20, 0]),
]


@pytest.mark.parametrize("start,order,want", HAND)
def test_hand_written_message_buffers(start, order, want):
    want = np.array(want, np.float32)
    got = ir.message_buffer(CANON, start[0], start[1], order)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(ir.canonical_from_message(want, 3, 4, start[0], start[1], order), CANON)


@pytest.mark.parametrize("rows,cols", ir.SHAPES)
def test_round_trip_for_every_shape_start_index_and_order(rows, cols):
    canon = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols)  # every cell its own value
    for si, sj in ir.start_indices(rows, cols):
        for order in ("row", "col"):
            buf = ir.message_buffer(canon, si, sj, order)
            assert buf.shape == ((rows, cols) if order == "row" else (rows * cols,))
            assert np.array_equal(ir.canonical_from_message(buf, rows, cols, si, sj, order), canon), (si, sj, order)
            # canonical (0, 0) and the last cell, addressed by hand
            flat = buf.reshape(-1)
            k0 = si * cols + sj if order == "row" else sj * rows + si
            bi, bj = (rows - 1 + si) % rows, (cols - 1 + sj) % cols
            k1 = bi * cols + bj if order == "row" else bj * rows + bi
            assert flat[k0] == canon[0, 0] and flat[k1] == canon[-1, -1], (si, sj, order)


def test_start_indices_exist_in_their_shape():
    for rows, cols in ir.SHAPES:
        starts = ir.start_indices(rows, cols)
        assert starts[0] == (0, 0) and starts[-1] == (rows // 2, cols // 3) and len(set(starts)) == len(starts)
        assert all(0 <= si < rows and 0 <= sj < cols for si, sj in starts)
    assert len(ir.start_indices(129, 96)) == 5 and ir.start_indices(1, 70) == [(0, 0), (0, 28), (0, 69), (0, 23)]


def _cases():
    for rows, cols in ir.SHAPES:
        yield rows, cols, [ir.YAML_PAIR]
    yield ir.HISTORY_SHAPE + (ir.HISTORY_PAIRS,)
    for rows, cols in ir.CARRY_SHAPES:
        yield rows, cols, ir.HISTORY_PAIRS


@pytest.mark.parametrize("rows,cols,pairs", list(_cases()))
def test_every_category_at_every_place(rows, cols, pairs):
    starts = ir.start_indices(rows, cols)
    trav, elev, placed = ir.hostile_map(rows, cols, ir.RES, seed=rows * 1000 + cols, thr_pairs=pairs, starts=starts)
    assert trav.shape == elev.shape == (rows, cols) and trav.dtype == elev.dtype == np.float32
    # what the helper reports is what the arrays hold
    layers = {"trav": trav, "elev": elev}
    for i, j, layer, cat in placed:
        assert ir.category_holds(cat, layers[layer][i, j]), (i, j, layer, cat)
    assert ir.missing_categories(trav, elev, pairs, starts) == []
    all_places = ir.places(rows, cols, starts)
    n_trav = len(ir.trav_categories(pairs))
    if min(rows, cols) >= 32:  # nothing was too small to hold every category
        assert all(len(c) >= n_trav for c in all_places.values())
    else:  # degenerate maps: a place smaller than the list holds hostile cells only, and not all of one category
        cells = {(i, j): cat for i, j, layer, cat in placed if layer == "trav"}
        small = {name: c for name, c in all_places.items() if len(c) < n_trav}
        for name, c in small.items():
            cats = [cells.get((int(i), int(j))) for i, j in c]
            assert None not in cats and len(set(cats)) >= min(len(cats), 2), name
        single = {cells[(int(c[0, 0]), int(c[0, 1]))] for c in small.values() if len(c) == 1}
        assert not single or len(single) >= 2  # nor do the single-cell places all hold one category
    # the same call gives the same map
    again = ir.hostile_map(rows, cols, ir.RES, seed=rows * 1000 + cols, thr_pairs=pairs, starts=starts)
    assert np.array_equal(again[0].view(np.uint32), trav.view(np.uint32)) and np.array_equal(again[1].view(np.uint32), elev.view(np.uint32))


def test_missing_categories_notices_a_lost_edge():
    """The check itself: wipe one place and it reports that place."""
    rows, cols = 65, 63
    starts = ir.start_indices(rows, cols)
    trav, elev, _ = ir.hostile_map(rows, cols, ir.RES, seed=5, thr_pairs=[ir.YAML_PAIR], starts=starts)
    trav[:, cols - 1] = 1.0
    lost = ir.missing_categories(trav, elev, [ir.YAML_PAIR], starts)
    assert lost and {name for name, _, _ in lost} >= {"last column"}


def test_the_planes_of_minus_infinity_and_the_strict_compare():
    """What the categories are for, in numpy: -inf is below every threshold but not finite (D set, Df clear); a cell AT a threshold
    does not fail it, its lower neighbour does."""
    for t in ir.thresholds_of(ir.HISTORY_PAIRS):
        at, below, above = (ir.category_value(f"{k} {float(t)!r}") for k in ("at", "below", "above"))
        assert below < t == at < above and not at < t
        assert np.nextafter(below, np.float32(np.inf)) == t == np.nextafter(above, np.float32(-np.inf))
    ninf = ir.category_value("-inf")
    assert all(ninf < t for t in ir.thresholds_of(ir.HISTORY_PAIRS)) and not np.isfinite(ninf)
    assert ir.category_value("denormal") > 0 and ir.category_value("denormal") < np.finfo(np.float32).tiny
