"""The argument block of the 3x3-only 8-lane kernels (plan_bits_kernel<NRL, true, kProd>, csrc/fpe_bits_lane8.hpp): those kernels
take PlanMidConsts, a cut of the call's PlanConsts, and read part of it again from the argument segment inside the cycle loop
(the flush every eighth cycle, the general leg search).  A field that is dropped, mis-copied or read at a wrong offset shows
where it is used, so the cases go there: batch edges of the two-pose wavefront, cycle counts around the eight-cycle flush,
every product shape, the per-leg radius override (make_leg_static), the walk gait, poses at the map's edge (pose_status, the
submap gate, the general leg search) and two parameter sets planned alternately on one map.  Everything against the oracle;
each case asserts which kernel ran."""
import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi, synth
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_poses
from tests import util

pytestmark = pytest.mark.gpu

RES, ROWS, COLS = 0.02, 200, 180
# searchRadius 0.134 and 0.125 on a 2 cm map: seven rings both (ceil(R / res)), so both run in the 15 x 15 window of <2, true>
R_A, R_B, RF = 0.134, 0.125, 0.02
KERNEL = "plan_bits_kernel<2, true> (8 lanes per leg, 15 x 15 bit window"
SHAPES = [util.DEFAULT_PRODUCTS, ("selected_packed",), ("nominal", "cycle_ok"), ("centroid", "stance", "selected")]
assert [util.product_shape(p) for p in SHAPES] == [2, 1, 1, 0]


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    yield p
    p.set_max_leg_search_radius(0.0)
    p.close()


def set_params(planner, **kw):
    planner.params = _capi.params_yaml()
    for k, v in kw.items():
        planner.params[k] = v


@pytest.fixture(scope="module")
def world():
    """One map for the module; poses over and beyond its border, a quarter lattice-aligned, both gaits."""
    trav, elev = synth.rough_map(ROWS, COLS, RES, seed=9100, bad_frac=0.25, nan_frac=0.002, stair_period=1.1)
    rng = np.random.default_rng(9101)
    B = 24
    lx, ly = ROWS * RES, COLS * RES
    xs, ys = rng.uniform(-0.5 * lx - 0.3, 0.5 * lx - 0.4, B), rng.uniform(-0.5 * ly - 0.25, 0.5 * ly + 0.25, B)
    xs[:6], ys[:6] = np.round(xs[:6] / RES) * RES, np.round(ys[:6] / RES) * RES
    # the first three poses start inside the map, so that the batches of one, two and three poses do real work; the first walks
    # along the map's +y border (half width 1.8 m: its left legs' boxes and windows hang over the edge), so that every batch
    # and cycle count crosses the general leg search and its reload of the argument block
    xs[:3], ys[:3] = [-1.2, -0.9, -1.4], [1.62, -0.5, 0.1]
    poses = make_poses(np.column_stack([xs, ys, rng.uniform(-0.1, 0.1, B)]))
    poses["gait"] = rng.integers(0, 2, B)
    poses["gait"][:3] = [0, 1, 0]
    return trav, elev, poses


def check(planner, poses, n, products, ora, what):
    eng = planner.plan(poses, n, products=products)
    d = planner.describe_plan()
    try:
        util.assert_products_equal(eng, util.slice_plan(ora, poses.shape[0]), products)
    except AssertionError as e:
        raise AssertionError(f"{what}, B {poses.shape[0]}, n {n}, products {products}, {d}: {e}") from None
    return eng


@pytest.fixture(scope="module")
def oracle17(planner, world):
    """The oracle's plan of all poses over seventeen cycles with the first parameter set: shared, read-only."""
    trav, elev, poses = world
    set_params(planner, searchRadius=np.float32(R_A), footRadius=np.float32(RF))
    return {n: util.run_oracle(planner, trav, elev, RES, poses, n, threads=8) for n in (1, 8, 9, 17)}


@pytest.mark.parametrize("n", [1, 8, 9, 17])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_batch_edges_and_flush_counts_every_product_shape(planner, world, oracle17, B, n):
    """B 1 / 2 / 3: a wavefront with an empty slot, a full one, the padding pose of the last block.  1 / 8 / 9 / 17 cycles: a
    flush of one unit, a full batch, a batch and one, two batches and one."""
    trav, elev, poses = world
    set_params(planner, searchRadius=np.float32(R_A), footRadius=np.float32(RF))
    planner.gridmapCallback(trav, elev, RES)
    assert planner.describe_plan().startswith(KERNEL), planner.describe_plan()
    for products in SHAPES:
        check(planner, poses[:B], n, products, oracle17[n], "batch edge")


def test_whole_batch_edge_poses_both_gaits(planner, world, oracle17):
    """All poses, some of them outside the map or with windows over its border (pose_status, the submap's `ok`, the general leg
    search), trot and walk mixed in one wavefront."""
    trav, elev, poses = world
    set_params(planner, searchRadius=np.float32(R_A), footRadius=np.float32(RF))
    planner.gridmapCallback(trav, elev, RES)
    assert planner.describe_plan().startswith(KERNEL), planner.describe_plan()
    ora = oracle17[9]
    for products in SHAPES:
        check(planner, poses, 9, products, ora, "whole batch")
    nom = ora["nominal"]
    assert (ora["pose_status"] != 0).any() and (ora["pose_status"] == 0).any()
    assert (nom["source"] == 1).any() and (nom["source"] == 0).any() and (nom["valid"] == 0).any() and (ora["centroid"]["code"] > 0).any()
    near = (nom["row"] < 7) | (nom["col"] < 7) | (nom["row"] >= ROWS - 7) | (nom["col"] >= COLS - 7)
    assert (near & (nom["valid"] != 0)).any()


def test_walk_gait_pose(planner, world):
    """One walk-gait pose: four phases a cycle, one swing leg each."""
    trav, elev, poses = world
    one = poses[1:2].copy()
    assert one["gait"][0] == 1
    set_params(planner, searchRadius=np.float32(R_A), footRadius=np.float32(RF))
    planner.gridmapCallback(trav, elev, RES)
    assert planner.describe_plan().startswith(KERNEL), planner.describe_plan()
    ora = util.run_oracle(planner, trav, elev, RES, one, 9, threads=4)
    for products in SHAPES:
        check(planner, one, 9, products, ora, "walk")
    assert ora["cycle_ok"].any()


def test_per_leg_radius_override_in_the_same_window_class(planner, world):
    """leg_search_radius of single legs: the wavefront takes make_leg_static, which reads searchRadius, maxSearchRadius and the
    per-leg biases from the block; the overrides stay within seven rings, so the kernel stays."""
    trav, elev, poses = world
    p = poses[:3].copy()
    p["leg_search_radius"][0] = [0.0, 0.128, 0.0, 0.0]
    p["leg_search_radius"][2] = [0.09, 0.0, 0.0, 0.131]  # five rings on one leg: fewer than the usual search's sixteen-candidate head
    set_params(planner, searchRadius=np.float32(R_A), footRadius=np.float32(RF))
    planner.gridmapCallback(trav, elev, RES)
    assert planner.describe_plan().startswith(KERNEL), planner.describe_plan()
    ora = util.run_oracle(planner, trav, elev, RES, p, 9, threads=4)
    for products in SHAPES:
        check(planner, p, 9, products, ora, "radius override")
    assert planner.describe_plan().startswith(KERNEL), planner.describe_plan()


def test_two_parameter_sets_alternate_on_one_map(world):
    """Two planners' worth of parameters on the same map — another searchRadius of the same window class, another step length —
    planned alternately, twice: the block is filled for each call from that call's constants."""
    trav, elev, poses = world
    sets = [dict(searchRadius=np.float32(R_A), footRadius=np.float32(RF)),
            dict(searchRadius=np.float32(R_B), footRadius=np.float32(RF), stepLength=np.float32(0.14))]
    planners = [FootholdPlanner(0), FootholdPlanner(0)]
    try:
        oras = []
        for pl, kw in zip(planners, sets):
            set_params(pl, **kw)
            pl.gridmapCallback(trav, elev, RES)
            assert pl.describe_plan().startswith(KERNEL), pl.describe_plan()
            oras.append(util.run_oracle(pl, trav, elev, RES, poses[:8], 9, threads=8))
        assert not np.array_equal(oras[0]["nominal"]["row"], oras[1]["nominal"]["row"])  # the two sets plan differently
        for _ in range(2):
            for pl, ora in zip(planners, oras):
                check(pl, poses[:8], 9, util.DEFAULT_PRODUCTS, ora, "alternating")
                check(pl, poses[:8], 9, ("selected_packed",), ora, "alternating")
        # and one planner whose parameters change between calls
        pl = planners[0]
        for kw, ora in list(zip(sets, oras)) * 2:
            set_params(pl, **kw)
            pl.gridmapCallback(trav, elev, RES)
            assert pl.describe_plan().startswith(KERNEL), pl.describe_plan()
            check(pl, poses[:8], 9, util.DEFAULT_PRODUCTS, ora, "re-parameterised")
    finally:
        for pl in planners:
            pl.close()


# one NRL 3 and one NRL 4 row of tests/test_gpu_plan_matrix.py's table: (res, searchRadius, footRadius, rows, cols, kernel)
WIDE = [
    ("w8_mid", 0.02, 0.154, 0.02, 200, 180, "plan_bits_kernel<3, true> (8 lanes per leg, 17 x 17 bit window"),
    ("w12_mid", 0.01, 0.117, 0.0095, 400, 360, "plan_bits_kernel<4, true> (8 lanes per leg, 25 x 25 bit window"),
]


@pytest.mark.parametrize("case", WIDE, ids=[c[0] for c in WIDE])
def test_three_and_four_rows_per_lane(planner, case):
    name, res, R, rf, rows, cols, kernel = case
    rng = np.random.default_rng(9200 + rows)
    trav, elev = synth.rough_map(rows, cols, res, seed=9300 + rows, bad_frac=0.25, nan_frac=0.002, stair_period=1.1)
    B = 11
    lx, ly = rows * res, cols * res
    xs, ys = rng.uniform(-0.5 * lx - 0.3, 0.5 * lx - 0.4, B), rng.uniform(-0.5 * ly - 0.25, 0.5 * ly + 0.25, B)
    poses = make_poses(np.column_stack([xs, ys, rng.uniform(-0.1, 0.1, B)]))
    poses["gait"] = rng.integers(0, 2, B)
    set_params(planner, searchRadius=np.float32(R), footRadius=np.float32(rf))
    planner.gridmapCallback(trav, elev, res)
    assert planner.describe_plan().startswith(kernel), (name, planner.describe_plan())
    ora = util.run_oracle(planner, trav, elev, res, poses, 9, threads=8)
    for products in SHAPES:
        check(planner, poses, 9, products, ora, name)
    assert (ora["nominal"]["source"] == 1).any() and (ora["centroid"]["code"] > 0).any()
