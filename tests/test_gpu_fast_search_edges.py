"""The straight-line leg search of the 3x3-only 8-lane kernels (leg_fast8m, csrc/fpe_bits_lane8.hpp) where its short cuts can go
wrong: the sixteen-candidate search for every rank and for none, windows that reach over each edge of the map while both 3x3
boxes stay inside it (the search no longer masks the cells outside the map: the sixteen candidates lie inside whenever the boxes
do), the disc box's column boundaries — where the y entry's "centre column is the box's middle column" flag decides —, and the
stance centre computed once for the first cycle's gate and for cycle 0.
Maps of 96 x 96 cells at 2 cm.  Every case: all products against the oracle (tests/util.py: indices / flags / x / y bit-exact,
|dz| <= 1e-6) and byte for byte against the direct kernels (no_bits = 1) on the same inputs.  What the inputs must contain — every
rank chosen, windows over every edge, the box boundaries, failing and passing gates — is asserted on the oracle's plan."""
import functools

import numpy as np
import pytest

from oracle import fpo
from quadrupedal_foothold_planner_amd import _capi, synth
from quadrupedal_foothold_planner_amd.planner import make_poses, make_strides

from tests import util

pytestmark = pytest.mark.gpu

RES, N = 0.02, 96
HALF = 0.5 * N * RES
X_C, Y_C = synth.cell_centres(N, N, RES)
# (searchRadius, the start of describe_plan(), window half-width): 11 x 11, 17 x 17 and 25 x 25 windows, two / three / four rows per lane
CLASSES = {"nrl2": (0.09, "plan_bits_kernel<2, true> (8 lanes per leg, 11 x 11 bit window", 5),
           "nrl3": (0.154, "plan_bits_kernel<3, true> (8 lanes per leg, 17 x 17 bit window", 8),
           "nrl4": (0.234, "plan_bits_kernel<4, true> (8 lanes per leg, 25 x 25 bit window", 12)}
SHAPES = {2: util.DEFAULT_PRODUCTS, 1: ("nominal", "cycle_ok"), 0: ("centroid", "stance", "selected")}
assert all(util.product_shape(p) == k for k, p in SHAPES.items())
LEG = 0  # the leg whose neighbourhood the rank map shapes


def class_params(cls):
    p = _capi.params_yaml()
    p["searchRadius"] = np.float32(CLASSES[cls][0])
    p["footRadius"] = np.float32(0.02)
    return p


def oracle_plan(params, trav, elev, poses, n, threads=4):
    omap = fpo.OracleMap(trav, elev, RES)
    op, opo = util.to_oracle_params(params), util.to_oracle_poses(poses)
    ora = omap.plan(op, opo, n, threads=threads)
    ora["pose_status"] = omap.pose_status(op, opo)
    return ora


@functools.lru_cache(maxsize=None)
def y_probe():
    """ny - y0 of every leg in cycle 0 (the default track's y is the leg centre's y: pose y + bias, no drift yet)."""
    trav, elev = synth.flat_map(N, N)
    d = oracle_plan(class_params("nrl2"), trav, elev, make_poses([[-0.2, 0.0, 0.0]]), 1)["default"]
    return d[0, 0, :, 1].copy()


# ---- 1. every rank and none ------------------------------------------------------------------------------------------------------
def rank_poses():
    """Eighteen poses on a 3 x 6 lattice.  Leg 0's centre lies a twentieth of a cell off its cell's centre in y — the whole 5 x 5
    neighbourhood is inside even the narrowest search rectangle (2.25 cells to either side) — and for pose 17 a third of a cell
    off, which leaves the far column of the neighbourhood outside that rectangle."""
    xs, js = np.meshgrid([-0.55, -0.2, 0.15], 8 + 16 * np.arange(6), indexing="ij")
    ys = Y_C[js.ravel()] - y_probe()[LEG] + 0.05 * RES
    ys[17] -= 0.4 * RES
    return make_poses(np.column_stack([xs.ravel(), ys, np.zeros(18)]))


@functools.lru_cache(maxsize=None)
def rank_world(cls):
    """The map: good everywhere but in the 5 x 5 neighbourhood of leg 0's default cell of every pose, where exactly the cell of
    spiral rank r passes for pose r < 16, none for pose 16, and for pose 17 the lowest-ranked cell that lies outside the search
    rectangle (when the class has one: the rectangle is searchRadius wide in y) together with one later cell inside it.
    Returns (trav, elev, poses, want, whether pose 17 has a cell outside): want[r] = the cell the search must choose in cycle 0; for
    pose 16 the centre cell, which it must stay three rings (rank 25) or more away from."""
    params, poses = class_params(cls), rank_poses()
    R = float(params["searchRadius"][0])
    trav, elev = synth.flat_map(N, N)
    elev += (0.001 * np.arange(N * N, dtype=np.float32).reshape(N, N) % 0.05).astype(np.float32)
    free = oracle_plan(params, trav, elev, poses, 1)["nominal"][:, 0, LEG]
    assert (free["source"] == 0).all() and (free["valid"] == 1).all()
    omap = fpo.OracleMap(trav, elev, RES)
    want = []
    for r in range(18):
        ci, cj, ny = int(free["row"][r]), int(free["col"][r]), float(free["y"][r])
        cells = [tuple(int(v) for v in c) for c in np.asarray(omap.spiral_cells(float(free["x"][r]), ny, R))[:16]]
        assert cells[0] == (ci, cj) and all(abs(i - ci) <= 2 and abs(j - cj) <= 2 for i, j in cells)
        trav[ci - 2:ci + 3, cj - 2:cj + 3] = 0.0
        if r < 16:
            trav[cells[r]] = 1.0
            want.append(cells[r])
        elif r == 16:
            want.append((ci, cj))
        else:
            outside = [q for q, (i, j) in enumerate(cells) if not (ny - 0.5 * R <= Y_C[j] < ny + 0.5 * R)]
            if outside:  # the cell outside would win by rank; the first cell inside that ranks behind it must
                q0 = outside[0]
                q1 = next(q for q in range(q0 + 1, 16) if q not in outside)
                trav[cells[q0]] = 1.0
                trav[cells[q1]] = 1.0
                want.append(cells[q1])
            else:
                trav[cells[9]] = 1.0
                want.append(cells[9])
    return trav, elev, poses, want, bool(outside)


def check_rank_world(cls):
    """The oracle on the rank map (runs without a GPU): all sixteen ranks chosen as intended, none for pose 16."""
    trav, elev, poses, want, has_outside = rank_world(cls)
    nom = oracle_plan(class_params(cls), trav, elev, poses, 1)["nominal"][:, 0, LEG]
    for r in range(18):
        if r == 16:
            ring = max(abs(int(nom["row"][r]) - want[r][0]), abs(int(nom["col"][r]) - want[r][1]))
            assert nom["valid"][r] == 0 or (nom["source"][r] == 1 and ring >= 3), (cls, r, nom[r])
        else:
            assert nom["valid"][r] == 1 and nom["source"][r] == 1 and (int(nom["row"][r]), int(nom["col"][r])) == want[r], (cls, r, nom[r], want[r])
    if cls == "nrl2":
        assert has_outside, "the narrowest rectangle must leave a cell of the 5 x 5 neighbourhood outside"
    return nom


@pytest.fixture(scope="module")
def planner():
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner

    p = FootholdPlanner(0)
    yield p
    p.set_max_leg_search_radius(0.0)
    p.set_tuning(no_bits=0)
    p.close()


def assert_bytes_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), f"{what}: {k} differs from the direct kernels"


def check(planner, params, kernel, trav, elev, poses, n, ora=None, products=util.DEFAULT_PRODUCTS, strides=None):
    """Engine against the oracle (`ora`, or planned here) and against the direct kernels; returns (engine's plan, oracle's plan)."""
    planner.params = params.copy()
    planner.gridmapCallback(trav, elev, RES)
    d = planner.describe_plan(strides=strides is not None)
    assert d.startswith(kernel), d
    eng = planner.plan(poses, n, products=products, strides=strides)
    if ora is None:
        ora = oracle_plan(params, trav, elev, poses, n)
    what = f"B {poses.shape[0]}, n {n}, {d}"
    try:
        if tuple(products) == util.DEFAULT_PRODUCTS:
            util.assert_plan_equal(eng, ora)
        else:
            util.assert_products_equal(eng, ora, products)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    with planner.tuning(no_bits=1):
        assert "direct" in planner.describe_plan(strides=strides is not None)
        direct = planner.plan(poses, n, products=products, strides=strides)
    assert_bytes_equal(eng, direct, what)
    return eng, ora


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_every_rank_and_none(planner, cls, n):
    """Pose r < 16: the first passing candidate of leg 0 in cycle 0 is the cell of spiral rank r; pose 16: none of the sixteen
    (the general candidate search takes over); pose 17: a passing cell outside the search rectangle must lose.  All three
    compiled product shapes."""
    check_rank_world(cls)
    trav, elev, poses, want, _ = rank_world(cls)
    params = class_params(cls)
    ora = oracle_plan(params, trav, elev, poses, n)
    for kprod in (2, 1, 0):
        check(planner, params, CLASSES[cls][1], trav, elev, poses, n, ora=ora, products=SHAPES[kprod])


# ---- 2. windows over each edge, boxes inside; 3. the disc box's column boundaries -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def speckled_map():
    """A third of the cells fail the default test only (0.8), nearly half fail both (0.5), the rest pass; a few unknown: most
    default discs fail and the first passing candidate is a different one from leg to leg."""
    rng = np.random.default_rng(9701)
    trav = rng.choice(np.array([0.8, 0.5, 1.0, np.nan], np.float32), size=(N, N), p=[0.33, 0.45, 0.2, 0.02])
    elev = rng.uniform(-0.05, 0.05, size=(N, N)).astype(np.float32)
    elev[np.isnan(trav)] = np.nan
    return trav, elev


INNER = (-0.21, 0.013)  # the interior pose every edge pose shares its wavefront with


def edge_poses(edge):
    """Poses in one-cell steps towards one edge (or a corner) of the map, from a window's reach inside it to legs outside, each
    followed by the interior pose: (edge pose, interior pose) is one wavefront."""
    k = np.arange(-3, 15)
    front, rear, side = HALF - 0.35 - RES * k, -HALF + 0.09 + RES * k, HALF - 0.0875 - 0.006 - RES * k
    xy = {"top": [(x, 0.10) for x in front], "bottom": [(x, -0.10) for x in rear], "left": [(-0.2, y) for y in side],
          "right": [(-0.2, -y) for y in side], "corner": [(x, y) for x in front[4:13:2] for y in side[4:13:2]]}[edge]
    both = np.array([p for e in xy for p in (e, INNER)])
    return make_poses(np.column_stack([both, np.zeros(len(both))]))


@pytest.mark.parametrize("cls", ["nrl2", "nrl3"])
@pytest.mark.parametrize("edge", ["top", "bottom", "left", "right", "corner"])
def test_window_over_each_edge_boxes_inside(planner, cls, edge):
    """Leg centres from outside the map to a window's reach inside it, default discs failing: the window crosses the edge while
    the boxes are inside (the straight-line search over a clipped window) and while they are not (the general leg search).  The
    interior pose's records are the same bytes in every wavefront, whichever way its neighbour sends the wavefront."""
    trav, elev = speckled_map()
    params, (_, kernel, winH) = class_params(cls), CLASSES[cls]
    poses = edge_poses(edge)
    eng, ora = check(planner, params, kernel, trav, elev, poses, 2)
    nom = ora["nominal"][0::2]
    near = {"top": nom["row"] <= winH, "bottom": nom["row"] >= N - 1 - winH, "left": nom["col"] <= winH, "right": nom["col"] >= N - 1 - winH,
            "corner": (nom["row"] <= winH) & (nom["col"] <= winH)}[edge]
    inside = (nom["row"] >= 2) & (nom["row"] <= N - 3) & (nom["col"] >= 2) & (nom["col"] <= N - 3)
    assert (near & inside & (nom["source"] == 1)).sum() >= 4, "candidate searches with the window over the edge and the boxes inside"
    assert (nom["valid"] == 0).any() or (ora["centroid"]["code"][0::2] == 6).any(), "legs at or beyond the edge"
    for k in eng:
        inner = eng[k][1::2]
        assert all(np.ascontiguousarray(inner[i]).tobytes() == np.ascontiguousarray(inner[0]).tobytes() for i in range(len(inner))), k


def test_y_flag_boundaries(planner):
    """The disc box's first column 0 and 1, its last column cols - 1 and past it, on either side of the map; and a leg whose y
    lies on a cell boundary to the last bit, where the box (two foot radii just short of two cells wide) has two columns, not
    three."""
    trav, elev = speckled_map()
    params, (_, kernel, _) = class_params("nrl2"), CLASSES["nrl2"]
    off = y_probe()
    ys = []
    for leg, sign in ((int(np.argmax(off)), 1.0), (int(np.argmin(off)), -1.0)):  # the leg nearest to either edge: its column 0 .. 4 from it
        ys += [sign * (HALF - (c + 0.4) * RES) - off[leg] for c in range(5)]
    boundary = Y_C[40] - 0.5 * RES  # between columns 40 and 41
    ys += [boundary - off[0], np.nextafter(boundary, 1.0) - off[0], boundary - off[1] + 1e-10]
    poses = make_poses(np.column_stack([np.full(len(ys), -0.2), ys, np.zeros(len(ys))]))
    eng, ora = check(planner, params, kernel, trav, elev, poses, 9)
    ny0 = ora["default"][:, 0, :, 1]
    cols = np.array([np.argmin(np.abs(Y_C - v)) for v in ny0.ravel()]).reshape(ny0.shape)
    for c in (0, 1, 2, 3, N - 4, N - 3, N - 2, N - 1):
        assert (cols == c).any(), f"no leg centre in column {c}"
    assert (np.abs(ny0[10:] - boundary) < 4e-10).any(), "a leg centre within the foot radius' deficit (4.5e-10 m) of a cell boundary: a two-column box"
    check(planner, params, kernel, trav, elev, poses, 1, products=SHAPES[1])


# ---- 4. the stance centre --------------------------------------------------------------------------------------------------------
def gate_poses():
    """Pose 0 passes the first cycle's gate, pose 1 fails it (the isosceles box reaches over the +x edge), pose 2 passes."""
    return make_poses([[-0.2, 0.05, 0.0], [HALF - 0.02, -0.31, 0.01], [0.1, 0.2, -0.02]])


@pytest.mark.parametrize("n", [1, 8, 9])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_stance_centre_gate_and_cycle0(planner, B, n):
    """pose_status, stance and cycle 0 of all three tracks: one pose and an empty slot, a failing gate beside a passing one,
    the padding slot of an odd batch; cycle counts on both sides of the flush."""
    trav, elev = speckled_map()
    params, (_, kernel, _) = class_params("nrl2"), CLASSES["nrl2"]
    poses = gate_poses()[:B]
    for kprod in (2, 0):
        eng, ora = check(planner, params, kernel, trav, elev, poses, n, products=SHAPES[kprod])
    want = [0, _capi.FPE_POSE_OPT_SUBMAP_FAILED, 0][:B]
    assert ora["pose_status"].tolist() == want, ora["pose_status"]
    assert ora["cycle_ok"][:, 0].any()


def test_stance_centre_in_the_general_copy(planner):
    """A trot pose and a walk-gait pose in one wavefront, a pose overriding one leg's radius beside the failing gate in the next,
    and the padding slot: the general copy of the body takes the shared centre in the first PHASE only."""
    trav, elev = speckled_map()
    params, (_, kernel, _) = class_params("nrl2"), CLASSES["nrl2"]
    poses = make_poses(np.concatenate([gate_poses()["position"], [[-0.3, -0.4, 0.0], [-0.05, 0.5, 0.0]]]))
    poses["gait"][[1, 3]] = 1
    poses["leg_search_radius"][2, 1] = np.float32(0.08)
    try:
        planner.set_max_leg_search_radius(0.09)
        for n in (1, 9):
            eng, ora = check(planner, params, kernel, trav, elev, poses, n)
    finally:
        planner.set_max_leg_search_radius(0.0)
    assert ora["pose_status"][1] == _capi.FPE_POSE_OPT_SUBMAP_FAILED and ora["cycle_ok"][[0, 2], 0].all()


def test_stance_centre_with_per_pose_strides(planner):
    """The stride entry points (host and device form) with two step lengths in one wavefront: the gate and cycle 0 use the pose's
    own step.  Reference: one oracle plan per pose with its stride."""
    from tests import stride_reference as sref
    from tests.test_gpu_strides import device_plan
    import torch

    trav, elev = speckled_map()
    params = class_params("nrl2")
    poses = gate_poses()
    poses["position"][1, 0] = HALF - 0.10  # (passes the gate with the short step, fails it with the long one)
    poses = poses[[0, 1, 1, 2]]
    strides = make_strides(np.array([0.18, 0.06, 0.26, 0.11], np.float32), np.array([-0.007, 0.0, 0.004, -0.007]))
    omap = fpo.OracleMap(trav, elev, RES)
    for n in (1, 9):
        ref = sref.plan_with_strides(omap, util.to_oracle_params(params), util.to_oracle_poses(poses), strides, n)
        eng, _ = check(planner, params, "plan_bits_kernel<2, false> stride", trav, elev, poses, n, ora=ref, strides=strides)
        dev = device_plan(planner, poses, strides, n, torch.cuda.Stream())
        assert_bytes_equal({k: dev[k] for k in eng}, eng, f"device form, n {n}")
    assert ref["pose_status"][1] == 0 and ref["pose_status"][2] == _capi.FPE_POSE_OPT_SUBMAP_FAILED
    assert not np.array_equal(ref["default"][1, 0], ref["default"][2, 0])
