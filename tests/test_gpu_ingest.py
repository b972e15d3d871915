"""Map ingest and the bit-plane cache (fpe_upload_map*, canonicalise_layer_kernel, build_bitmap_kernel, acquire_mask) against the
oracle on the CANONICAL arrays: every message layout (row- and column-major, circular-buffer start index), host and device
sources, the planes of both builders, and the history of threshold pairs on one snapshot and across uploads.  The maps are
tests/ingest_reference.py's hostile maps — every special value at every edge, last word, last row group and wrap — with at most
16 384 cells, and EVERY cell is compared.

The observers:
  1. foothold_map() with the yaml footRadius reads the bit planes: flags equal, heights bit for bit;
  2. foothold_map() with footRadius 0 reads the two float layers, one cell per disc: the same bar;
  3. a batch plan of 48 poses x 4 cycles, a third of them placed by hand against the edges and corners: the project's bar
     (util.assert_plan_equal), on a plan_bits_* kernel;
  4. where one snapshot content is reached by two routes, observers 1 and 2 are byte-identical between them (each side is also
     compared with the oracle)."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import fpo
from quadrupedal_foothold_planner_amd import _capi, synth
from quadrupedal_foothold_planner_amd.planner import PRODUCT_FIELDS, FootholdPlanner, PlanOut, make_poses, product_shapes
from tests import ingest_reference as ir
from tests import util
from tests.test_gpu_filters import assert_layers_equal, assert_no_threshold_crossing, assert_traversability_only
from tests.test_gpu_foothold_map import all_cells, oracle_cells

pytestmark = pytest.mark.gpu

RES = ir.RES
N_CYCLES = 4
NEW_PAIR = (0.9, 0.85)  # (case D) a pair no snapshot has seen; it shares its default threshold with pair 1, which is carried


def params_for(pair, foot_radius=None):
    p = _capi.params_yaml()
    p["defaultFootholdThreshold"], p["candidateFootholdThreshold"] = np.float32(pair[0]), np.float32(pair[1])
    if foot_radius is not None:
        p["footRadius"] = np.float32(foot_radius)
    return p


def edge_poses(rows, cols, seed, B=48):
    """A third by hand: towards each edge and corner, a pose whose outer feet stand 3 cm inside the map's edge and one whose outer
    feet stand 4 cm outside it — within one search radius (0.1) either way, so their search windows hang over the edge.  The
    others anywhere up to 10 cm outside the map."""
    p = _capi.params_yaml()
    hx, hy = 0.5 * rows * RES, 0.5 * cols * RES
    fx, fy = 0.5 * float(p["length"][0]), 0.5 * float(p["width"][0])
    hand = [(sx * (hx - fx - d), sy * (hy - fy - d), 0.0) for sx in (-1, 0, 1) for sy in (-1, 0, 1) if (sx, sy) != (0, 0) for d in (0.03, -0.04)]
    assert len(hand) == B // 3
    rng = np.random.default_rng(seed)
    rest = np.column_stack([rng.uniform(-hx - 0.1, hx + 0.1, B - len(hand)), rng.uniform(-hy - 0.1, hy + 0.1, B - len(hand)),
                            rng.uniform(-0.1, 0.1, B - len(hand))])
    return make_poses(np.concatenate([np.array(hand), rest]))


class Reference:
    """A canonical map with the oracle's answers on it, each computed once and shared."""

    def __init__(self, rows, cols, seed, pairs):
        self.rows, self.cols = rows, cols
        self.starts = ir.start_indices(rows, cols)
        self.trav, self.elev, self.placed = ir.hostile_map(rows, cols, RES, seed, pairs, self.starts)
        assert ir.missing_categories(self.trav, self.elev, pairs, self.starts) == []
        self.omap = fpo.OracleMap(self.trav, self.elev, RES)
        self.poses = edge_poses(rows, cols, seed + 1)
        self._cells, self._plans, self._messages = {}, {}, {}
        self.first = None  # observers 1 and 2 of the first route that reached this content (observer 4)

    def cells(self, pair, foot_radius=None):
        """{"flags", "height"} [rows, cols] of the oracle for every cell."""
        key = (np.float32(pair[0]).tobytes(), np.float32(pair[1]).tobytes(), foot_radius)
        if key not in self._cells:
            f, h = oracle_cells(self.omap, params_for(pair, foot_radius), all_cells(self.rows, self.cols))
            self._cells[key] = {"flags": f.reshape(self.rows, self.cols), "height": h.reshape(self.rows, self.cols)}
        return self._cells[key]

    def plan(self, pair, poses=None, n_cycles=N_CYCLES):
        key = (pair, None if poses is None else poses.tobytes(), n_cycles)
        if key not in self._plans:
            op, opo = util.to_oracle_params(params_for(pair)), util.to_oracle_poses(self.poses if poses is None else poses)
            ora = self.omap.plan(op, opo, n_cycles, threads=8)
            ora["pose_status"] = self.omap.pose_status(op, opo)
            self._plans[key] = ora
        return self._plans[key]

    def message(self, start, order):
        """(traversability, elevation) in the message's layout, as gridmapCallback takes them."""
        key = (start, order)
        if key not in self._messages:
            bufs = [ir.message_buffer(a, start[0], start[1], order) for a in (self.trav, self.elev)]
            for b, a in zip(bufs, (self.trav, self.elev)):
                back = ir.canonical_from_message(b, self.rows, self.cols, start[0], start[1], order)
                assert np.array_equal(back.view(np.uint32), a.view(np.uint32))
            self._messages[key] = [b if order == "row" else b.reshape(self.cols, self.rows) for b in bufs]
        return self._messages[key]


_REFERENCES = {}


def reference(rows, cols, kind="layout"):
    """layout: the yaml pair's categories; history / carry / other: those of the six pairs of the pair history."""
    key = (rows, cols, kind)
    if key not in _REFERENCES:
        seed = rows * 1000 + cols + {"layout": 0, "history": 1, "carry": 2, "other": 3}[kind]
        _REFERENCES[key] = Reference(rows, cols, seed, [ir.YAML_PAIR] if kind == "layout" else ir.HISTORY_PAIRS)
    return _REFERENCES[key]


def assert_cells_equal(got, want, what):
    """assert_cells' bar (tests/test_gpu_foothold_map.py) on whole arrays: flags equal, heights bit for bit, every cell."""
    assert got["flags"].shape == want["flags"].shape and got["height"].shape == want["height"].shape, what
    bad = np.argwhere(got["flags"] != want["flags"])
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} flag mismatches, first at {tuple(bad[0])}: {got['flags'][tuple(bad[0])]} != {want['flags'][tuple(bad[0])]}"
    bad = np.argwhere(got["height"].view(np.uint32) != want["height"].view(np.uint32))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} height mismatches, first at {tuple(bad[0])}: {got['height'][tuple(bad[0])]!r} != {want['height'][tuple(bad[0])]!r}"


def assert_same_bytes(a, b, what):
    for k in ("bits", "layers"):
        assert np.array_equal(a[k]["flags"], b[k]["flags"]), f"{what}: {k} flags differ between two routes to one snapshot content"
        assert np.array_equal(a[k]["height"].view(np.uint32), b[k]["height"].view(np.uint32)), f"{what}: {k} heights differ between two routes"


# ---- uploads and observers, host form ------------------------------------------------------------------------------------------------
def upload_host(planner, ref, start=(0, 0), order="row"):
    t, e = ref.message(start, order)
    planner.gridmapCallback(t, e, RES, start_index=start, storage_order=order)


def observe_host(planner, pair, poses=None, layers=True):
    """Observers 1 and 3, and 2 with `layers`, on the current snapshot."""
    planner.params = params_for(pair)
    out = {"bits": planner.foothold_map(), "kernel": planner.describe_plan()}
    if poses is not None:
        out["plan"] = planner.plan(poses, N_CYCLES)
    if layers:
        planner.params = params_for(pair, 0.0)
        out["layers"] = planner.foothold_map()
    return out


# ---- uploads and observers, device form: nothing here waits for the GPU ----------------------------------------------------------------
class DeviceSide:
    """torch owns the buffers and the two streams: uploads go to `up`, every observer to `side`."""

    def __init__(self):
        import torch

        self.torch = torch
        self.up, self.side = torch.cuda.Stream(), torch.cuda.Stream()
        self.keep = []

    def upload(self, planner, ref, start=(0, 0), order="row"):
        torch = self.torch
        t, e = ref.message(start, order)
        d_t, d_e = torch.from_numpy(t.reshape(-1)).cuda(), torch.from_numpy(e.reshape(-1)).cuda()
        torch.cuda.synchronize()  # the sources are in HBM; from here on the host waits for nothing
        self.keep += [d_t, d_e]
        planner.upload_map_device(d_t.data_ptr(), d_e.data_ptr(), ref.rows, ref.cols, RES, start_index=start, storage_order=order,
                                  stream=self.up.cuda_stream)

    def poses(self, poses):
        d = self.torch.from_numpy(poses.view(np.uint8).reshape(-1).copy()).cuda()
        self.torch.cuda.synchronize()
        self.keep.append(d)
        return d

    def queue_map(self, planner, pair, shape, foot_radius=None):
        torch = self.torch
        n = shape[0] * shape[1]
        with torch.cuda.stream(self.side):
            d_f = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
            d_h = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        planner.params = params_for(pair, foot_radius)
        planner.foothold_map_device(d_f.data_ptr(), d_h.data_ptr(), stream=self.side.cuda_stream)
        return d_f, d_h

    def queue_plan(self, planner, pair, d_poses, B, n_cycles, stream=None):
        torch = self.torch
        stream = stream or self.side
        shapes = product_shapes(B, n_cycles)
        with torch.cuda.stream(stream):
            bufs = {k: torch.zeros(int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize, dtype=torch.uint8, device="cuda")
                    for k in util.DEFAULT_PRODUCTS}
        planner.params = params_for(pair)
        planner.plan_device(d_poses.data_ptr(), B, n_cycles, bufs["nominal"].data_ptr(), bufs["centroid"].data_ptr(),
                            bufs["default"].data_ptr(), bufs["cycle_ok"].data_ptr(), bufs["stance"].data_ptr(), stream=stream.cuda_stream,
                            d_selected_ptr=bufs["selected"].data_ptr(), d_pose_status_ptr=bufs["pose_status"].data_ptr())
        return bufs

    @staticmethod
    def fetch_map(d, shape):
        return {"flags": d[0].cpu().numpy().reshape(shape), "height": d[1].cpu().numpy().reshape(shape)}

    @staticmethod
    def fetch_plan(bufs, B, n_cycles):
        shapes = product_shapes(B, n_cycles)
        return {k: v.cpu().numpy().view(shapes[k][1]).reshape(shapes[k][0]) for k, v in bufs.items()}

    def observe(self, planner, ref, pair, d_poses):
        """Observers 1, 3 and 2 queued on `side` behind an upload on `up`; then the one wait, and the results."""
        shape = (ref.rows, ref.cols)
        bits = self.queue_map(planner, pair, shape)
        kernel = planner.describe_plan()
        plan = self.queue_plan(planner, pair, d_poses, ref.poses.shape[0], N_CYCLES)
        layers = self.queue_map(planner, pair, shape, 0.0)
        self.side.synchronize()
        self.up.synchronize()
        return {"bits": self.fetch_map(bits, shape), "kernel": kernel, "plan": self.fetch_plan(plan, ref.poses.shape[0], N_CYCLES),
                "layers": self.fetch_map(layers, shape)}


def check_observers(obs, ref, pair, what):
    assert_cells_equal(obs["bits"], ref.cells(pair), f"{what}, bit planes")
    if "layers" in obs:
        assert_cells_equal(obs["layers"], ref.cells(pair, 0.0), f"{what}, float layers")
    if "plan" in obs:
        assert "plan_bits_" in obs["kernel"], obs["kernel"]  # the planes are what the plan read
        util.assert_plan_equal(obs["plan"], ref.plan(pair))


# ---- A. layout x source x plane route ----------------------------------------------------------------------------------------------
def _layout_cases():
    for rows, cols in ir.FULL_SHAPES:
        for start in ir.start_indices(rows, cols):
            for order in ("row", "col"):
                for source in ("host", "device"):
                    yield rows, cols, start, order, source
    for rows, cols in ir.SHAPES:
        if (rows, cols) not in ir.FULL_SHAPES:
            for order in ("row", "col"):
                yield rows, cols, ir.start_indices(rows, cols)[-1], order, "host"


@pytest.mark.parametrize("rows,cols,start,order,source", list(_layout_cases()),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_layout_source_and_plane_route(rows, cols, start, order, source):
    """One message layout from one source, twice into a fresh engine: (i) no pair known, the first call builds the planes lazily
    (build_bitmap_kernel); (ii) the same upload again, now that the pair is registered: the planes come from the canonicalising
    kernel (or, for a canonical host array, from the upload's own build).  Both against the oracle, and byte-identical with each
    other and with every other route to this map."""
    ref = reference(rows, cols)
    if min(rows, cols) >= 32:  # the hand-placed poses do reach over all four edges: on the oracle's stance feet
        feet = ref.plan(ir.YAML_PAIR)["stance"][:16]
        hx, hy = 0.5 * rows * RES, 0.5 * cols * RES
        for axis, half in ((0, hx), (1, hy)):
            assert (np.abs(feet[:, :, axis] - half) < 0.1).any() and (np.abs(feet[:, :, axis] + half) < 0.1).any()
    planner = FootholdPlanner(0)
    try:
        dev = DeviceSide() if source == "device" else None
        d_poses = dev.poses(ref.poses) if dev else None
        routes = []
        for route in ("lazy planes", "planes of the upload"):
            what = f"{rows} x {cols}, start {start}, {order}-major, {source} source, {route}"
            if dev:
                dev.upload(planner, ref, start, order)
                obs = dev.observe(planner, ref, ir.YAML_PAIR, d_poses)
            else:
                upload_host(planner, ref, start, order)
                obs = observe_host(planner, ir.YAML_PAIR, ref.poses)
            check_observers(obs, ref, ir.YAML_PAIR, what)
            routes.append(obs)
        assert_same_bytes(routes[0], routes[1], what)
        if ref.first is None:
            ref.first = routes[0]
        assert_same_bytes(ref.first, routes[1], what)
    finally:
        planner.close()


# ---- B. the producer's elevation input through the same kernel ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.close()


@pytest.mark.parametrize("rows,cols", [(65, 63), (127, 100)])
def test_traversability_from_a_row_major_buffer_with_a_start_index(planner, rows, cols):
    _, elev = synth.rough_map(rows, cols, RES, seed=rows + cols)
    si, sj = rows // 2, cols // 3
    msg = ir.message_buffer(elev, si, sj, "row")
    assert np.array_equal(ir.canonical_from_message(msg, rows, cols, si, sj, "row").view(np.uint32), elev.view(np.uint32))
    trav_m, layers_m = planner.traversability_from_elevation(msg, RES, start_index=(si, sj), storage_order="row", want_layers=True)
    trav_c, layers_c = planner.traversability_from_elevation(elev, RES, want_layers=True)
    # the same input after canonicalisation, the same kernels: byte-identical
    assert np.array_equal(trav_m.view(np.uint32), trav_c.view(np.uint32))
    for name in _capi.FILTER_LAYERS:
        assert np.array_equal(layers_m[name].view(np.uint32), layers_c[name].view(np.uint32)), name
    only_m = planner.traversability_from_elevation(msg, RES, start_index=(si, sj), storage_order="row")
    only_c = planner.traversability_from_elevation(elev, RES)
    assert np.array_equal(only_m.view(np.uint32), only_c.view(np.uint32))
    # and the filter oracle, at the bar of tests/test_gpu_filters.py
    ora = fpo.traversability_filters(elev, RES)
    same_normal = assert_layers_equal(layers_m, ora)
    assert_traversability_only(only_m, layers_m, ora, same_normal)
    assert_no_threshold_crossing(trav_m, ora["traversability"])
    assert_no_threshold_crossing(only_m, ora["traversability"], "traversability only: ")


# ---- C. pair history on one snapshot -----------------------------------------------------------------------------------------------
# six pairs, then pair 1 again (evicted by the fifth: rebuilt), pair 6 (cached), pair 2 (evicted by the sixth).  A snapshot keeps
# four sets and evicts the least recently used, so this leaves pairs 5, 6, 1, 2 in it — pairs 3 and 4 went when 1 and 2 came back.
HISTORY = ir.HISTORY_PAIRS + [ir.HISTORY_PAIRS[0], ir.HISTORY_PAIRS[5], ir.HISTORY_PAIRS[1]]
CARRIED = [ir.HISTORY_PAIRS[4], ir.HISTORY_PAIRS[5], ir.HISTORY_PAIRS[0], ir.HISTORY_PAIRS[1]]
EVICTED = ir.HISTORY_PAIRS[2]


def history_reference():
    """The history map, with the check that makes a stale or swapped set visible: on the ORACLE's outputs, consecutive pairs
    give different flags in at least 1 % of the cells."""
    ref = reference(*ir.HISTORY_SHAPE, kind="history")
    assert (ref.trav == np.float32(ir.HISTORY_PAIRS[5][0])).any()  # pair 6 is a value present in the map
    for a, b in zip(HISTORY, HISTORY[1:]):
        assert (ref.cells(a)["flags"] != ref.cells(b)["flags"]).mean() >= 0.01, (a, b)
    return ref


def run_history(planner, ref, check):
    upload_host(planner, ref)
    for k, pair in enumerate(HISTORY):
        obs = observe_host(planner, pair, ref.poses if check else None, layers=False)
        if check:
            check_observers(obs, ref, pair, f"pair history, step {k + 1}: {pair}")


def test_pair_history_on_one_snapshot():
    ref = history_reference()
    planner = FootholdPlanner(0)
    try:
        run_history(planner, ref, check=True)
    finally:
        planner.close()


# ---- D. pairs carried across an upload ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", ir.CARRY_SHAPES)
@pytest.mark.parametrize("route", ["host row-major canonical", "host column-major start", "device row-major start", "device column-major start"])
def test_pairs_carried_across_an_upload_of_another_shape(route, rows, cols):
    """After the history, a map of another shape (more / fewer words per row: recycled plane buffers fit neither in content nor in
    stride).  The first carried pair's planes ride in the canonicalising kernel where the layer passes through one, the others are
    built by build_bitmap_kernel on the upload's stream: observer 1 for the four carried pairs, one evicted pair and one new pair,
    all against the oracle on the NEW map — in the device cases with no host synchronisation anywhere in between."""
    old, new = history_reference(), reference(rows, cols, kind="carry")
    pairs = CARRIED + [EVICTED, NEW_PAIR]
    r, c = min(old.rows, rows), min(old.cols, cols)
    for pair in pairs:  # the old planes would not pass for the new ones
        assert (old.cells(pair)["flags"][:r, :c] != new.cells(pair)["flags"][:r, :c]).any(), pair
    source, order = route.split(" ")[0], "row" if "row-major" in route else "col"
    start = (0, 0) if "canonical" in route else new.starts[-1]
    planner = FootholdPlanner(0)
    try:
        run_history(planner, old, check=False)
        if source == "host":
            upload_host(planner, new, start, order)
            got = [observe_host(planner, pair, layers=False)["bits"] for pair in pairs]
        else:
            dev = DeviceSide()
            dev.upload(planner, new, start, order)
            queued = [dev.queue_map(planner, pair, (rows, cols)) for pair in pairs]
            dev.side.synchronize()
            dev.up.synchronize()
            got = [dev.fetch_map(q, (rows, cols)) for q in queued]
        for pair, g in zip(pairs, got):
            assert_cells_equal(g, new.cells(pair), f"{route}, {rows} x {cols}, pair {pair}")
    finally:
        planner.close()


# ---- E. eviction while a call is in flight -------------------------------------------------------------------------------------------
def test_a_queued_plan_keeps_its_planes_through_an_eviction_and_an_upload():
    """plan_device with pair 1 queued on one stream; four new pairs on another evict pair 1's set; an upload of another map recycles
    buffers; only then the first stream is waited for.  Its products are the oracle's plan for pair 1 on the OLD map."""
    old, new = history_reference(), reference(*ir.CARRY_SHAPES[0], kind="carry")
    B, n = 4096, 8
    rng = np.random.default_rng(11)
    hx, hy = 0.5 * old.rows * RES, 0.5 * old.cols * RES
    poses = make_poses(np.column_stack([rng.uniform(-hx - 0.05, hx - 0.5, B), rng.uniform(-hy - 0.05, hy + 0.05, B), np.zeros(B)]))
    want = old.plan(ir.HISTORY_PAIRS[0], poses, n)
    assert want["cycle_ok"].any() and not want["cycle_ok"].all()
    planner = FootholdPlanner(0)
    try:
        dev = DeviceSide()
        d_poses = dev.poses(poses)
        upload_host(planner, old)
        plan = dev.queue_plan(planner, ir.HISTORY_PAIRS[0], d_poses, B, n, stream=dev.up)
        evictors = ir.HISTORY_PAIRS[1:5]
        queued = [dev.queue_map(planner, pair, (old.rows, old.cols)) for pair in evictors]
        upload_host(planner, new)
        after = observe_host(planner, ir.HISTORY_PAIRS[0], layers=False)["bits"]
        dev.up.synchronize()
        dev.side.synchronize()
        util.assert_plan_equal(dev.fetch_plan(plan, B, n), want)
        for pair, q in zip(evictors, queued):
            assert_cells_equal(dev.fetch_map(q, (old.rows, old.cols)), old.cells(pair), f"evicting pair {pair}")
        assert_cells_equal(after, new.cells(ir.HISTORY_PAIRS[0]), "pair 1 on the new map")
    finally:
        planner.close()


# ---- F. two host threads, two pairs, one uploader ------------------------------------------------------------------------------------
def plan_with(planner, params, poses, n_cycles, products=("nominal", "cycle_ok")):
    """fpe_plan with the caller's own parameter block (planner.params is shared between threads: not touched here)."""
    B = poses.shape[0]
    shapes = product_shapes(B, n_cycles)
    out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in products}
    po = PlanOut()
    for k in products:
        setattr(po, PRODUCT_FIELDS[k], _capi.ptr(out[k]))
    planner._check(planner._lib.fpe_plan(planner._h, _capi.ptr(params), _capi.ptr(poses), B, int(n_cycles), C.byref(po)))
    return out


def test_two_threads_with_their_own_pairs_while_maps_are_swapped():
    """Each snapshot is planned with two pairs at once and carries both into the next upload: every result is the oracle's plan for
    ITS pair on one of the two maps."""
    maps = [history_reference(), reference(*ir.HISTORY_SHAPE, kind="other")]
    pairs = [ir.HISTORY_PAIRS[0], ir.HISTORY_PAIRS[1]]
    poses = maps[0].poses
    products = ("nominal", "cycle_ok")
    want = [[m.plan(pair, poses) for m in maps] for pair in pairs]
    for k in (0, 1):  # nothing here can be taken for anything else
        assert not np.array_equal(want[k][0]["nominal"]["row"], want[k][1]["nominal"]["row"]), "the two maps must plan differently"
        assert not np.array_equal(want[0][k]["nominal"]["row"], want[1][k]["nominal"]["row"]), "the two pairs must plan differently"
    planner = FootholdPlanner(0)
    errors, seen = [], [[0, 0], [0, 0]]

    def uploader():
        try:
            for k in range(30):
                upload_host(planner, maps[(k + 1) & 1])
        except Exception as e:  # pragma: no cover
            errors.append(repr(e))

    def client(k):
        try:
            prm = params_for(pairs[k])
            for it in range(40):
                eng = plan_with(planner, prm, poses, N_CYCLES, products)
                which = []
                for m in (0, 1):
                    try:
                        util.assert_products_equal(eng, want[k][m], products)
                        which.append(m)
                    except AssertionError:
                        pass
                if not which:
                    errors.append(f"pair {pairs[k]}, plan {it}: the result is the oracle's on neither map")
                else:
                    seen[k][which[0]] += 1
        except Exception as e:  # pragma: no cover
            errors.append(repr(e))

    try:
        upload_host(planner, maps[0])
        ths = [threading.Thread(target=uploader)] + [threading.Thread(target=client, args=(k,)) for k in (0, 1)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errors, errors[:3]
        assert sum(seen[0]) == 40 and sum(seen[1]) == 40
        # the last upload carried both pairs: observer 1 for each, on the map that is current now
        for pair in pairs:
            assert_cells_equal(observe_host(planner, pair, layers=False)["bits"], maps[0].cells(pair), f"after the swaps, pair {pair}")
    finally:
        planner.close()
