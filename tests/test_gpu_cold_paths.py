"""The rare branches of the 3x3-only 8-lane plan kernels (csrc/fpe_bits_lane8.hpp), each driven both ways.
Every wave-uniform "this almost never happens" test of those kernels carries a branch weight (FPE_RARE, csrc/fpe_kernels.hip): the
compiler lays the cold body — the general leg search, the candidate search beyond rank 15, the division behind div3's range
guard, the reference's own corner expressions of the y fill and of the first cycle's gate, the priority hand-over — outside the
cycle loop and allocates registers for the straight path.  Layout must not change a result; what can go wrong is a cold body that
runs from another register or spill state than before.  So each guard is taken and not taken here, in one wavefront where that is
possible (the neighbour pose stays on the straight path), on the smallest shapes that reach it: maps of 96 x 96 cells at 2 cm,
search radius 0.1 (plan_bits_kernel<2, true, *>) with one sibling case each for the instances with three and four window rows per
lane, one / two / three poses (one live slot, two, a padding slot) and one / eight / nine cycles (a short batch, a full one, a
second short one).
Every case: against the oracle (tests/util.py: indices / flags / x / y bit-exact, |dz| <= 1e-6) and byte for byte against the
direct kernels (no_bits = 1), for all seven products and for the nominal-only product set.  That an input reaches its branch is
asserted on the oracle's plan and on the inputs (the *_inputs functions: they run without a GPU)."""
import functools

import numpy as np
import pytest

from oracle import fpo
from quadrupedal_foothold_planner_amd import _capi, synth
from quadrupedal_foothold_planner_amd.planner import make_poses

from tests import util
from tests.test_gpu_deferred_heights import border_walks, hostile_map, mixed_batches
from tests.test_gpu_fast_search_edges import HALF, INNER, N, RES, X_C, Y_C, check, oracle_plan, speckled_map

pytestmark = pytest.mark.gpu

RADIUS = {"nrl2": 0.1, "nrl3": 0.154, "nrl4": 0.234}
KERNEL = {c: f"plan_bits_kernel<{c[3]}, true> (8 lanes per leg" for c in RADIUS}
NOMINAL_ONLY = ("nominal", "selected", "cycle_ok")
assert util.product_shape(util.DEFAULT_PRODUCTS) == 2 and util.product_shape(NOMINAL_ONLY) == 1
BS, NS = (1, 2, 3), (1, 8, 9)
SHORT = 0.06  # a step length that keeps nine cycles of an interior pose inside the map


def params_of(cls="nrl2", step=None, drift=None):
    p = _capi.params_yaml()
    p["searchRadius"] = np.float32(RADIUS[cls])
    p["footRadius"] = np.float32(0.02)
    if step is not None:
        p["stepLength"] = np.float32(step)
    if drift is not None:
        p["lateralDrift"] = drift
    return p


@pytest.fixture(scope="module")
def planner():
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner

    p = FootholdPlanner(0)
    yield p
    p.set_max_leg_search_radius(0.0)
    p.set_tuning(no_bits=0)
    p.close()


def both(planner, params, cls, trav, elev, poses, n):
    """All seven products and the nominal-only set, each against the oracle and the direct kernels; returns the oracle's plan."""
    _, ora = check(planner, params, KERNEL[cls], trav, elev, poses, n)
    check(planner, params, KERNEL[cls], trav, elev, poses, n, ora=ora, products=NOMINAL_ONLY)
    return ora


def xyz(rows):
    return make_poses(np.array([[x, y, 0.0] for x, y in rows], np.float64))


def general_copy(poses):
    """`poses` beside a walk-gait pose and a pose that overrides one leg's search radius: every wavefront with one of the two takes
    the general copy of the body.  The two go BETWEEN the given poses, so that each shares a wavefront with one of them."""
    extra = xyz([(-0.3, -0.4), (-0.05, 0.5)])
    extra["gait"][0] = 1
    extra["leg_search_radius"][1, 1] = np.float32(0.08)
    out = []
    for k, p in enumerate(poses):
        out += [p, extra[k % 2]]
    return np.array(out, dtype=poses.dtype)


def run_general(planner, params, cls, trav, elev, poses, n):
    try:
        planner.set_max_leg_search_radius(RADIUS[cls])
        return both(planner, params, cls, trav, elev, general_copy(poses), n)
    finally:
        planner.set_max_leg_search_radius(0.0)


# ---- 1. the `rare` ballot of leg_fast8m ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def x_probe(cls="nrl2"):
    """default-track x of every leg in cycle 0, minus the pose's x (feet-polygon centre + step + the leg's bias)."""
    trav, elev = synth.flat_map(N, N)
    d = oracle_plan(params_of(cls, step=SHORT), trav, elev, xyz([(-0.2, 0.0)]), 1)["default"]
    return d[0, 0, :, 0] + 0.2


def corner_quotient(x):
    """the x pass's quotient of a box corner, in cells: the corner is ON a cell boundary where this is an integer"""
    return (x - HALF) / RES


@functools.lru_cache(maxsize=None)
def boundary_inputs(cls="nrl2"):
    """A pose whose leg 0 has the foot disc's corner cx + rf within 5e-13 cells of a cell boundary in cycle 0 (cornerEps is 1e-12
    and more: the x pass does not trust its predicted index there), by corrections of the pose's x on the oracle's answer."""
    params = params_of(cls, step=SHORT)
    trav, elev = hostile_map(N)
    rf = float(params["footRadius"][0])
    target = X_C[40] + 0.5 * RES  # the boundary between rows 39 and 40
    x0 = target - rf - x_probe(cls)[0]
    for _ in range(4):
        cx = oracle_plan(params, trav, elev, xyz([(x0, 0.013)]), 1)["default"][0, 0, 0, 0]
        x0 -= (cx + rf) - target
    pose = (x0, 0.013)
    cx = oracle_plan(params, trav, elev, xyz([pose]), 1)["default"][0, 0, 0, 0]
    q = corner_quotient(cx + rf)
    assert abs(q - round(q)) < 5e-13, (cls, q)
    return pose


@functools.lru_cache(maxsize=None)
def nan_centre_poses():
    """Poses whose centroid track reaches a NON-FINITE centre inside the chain, and one that never does.  (The engine refuses a
    non-finite pose as an argument error, so a NaN cannot enter by the pose; it arises where the centroid track has committed
    its "no case" results (0, 0, 0) for all four feet and the feet polygon has no area: 0 / 0, cpp:2421-2463.  On the speckled map
    most chains get there within a few cycles.)  Chosen on the oracle's plan: the nominal record of an unusable centre carries it."""
    rng = np.random.default_rng(5)
    cand = xyz(list(zip(rng.uniform(-0.7, 0.0, 64), rng.uniform(-0.6, 0.6, 64))))
    x = oracle_plan(params_of(step=SHORT), *speckled_map(), cand, 9)["nominal"]["x"]
    first = np.array([np.argmax(np.isnan(x[i]).any(axis=1)) if np.isnan(x[i]).any() else -1 for i in range(64)])
    late = np.nonzero((first >= 2) & (first <= 6))[0]  # finite cycles first: the flip is inside the first batch
    never = np.nonzero(first < 0)[0]
    assert late.size >= 2 and never.size >= 1
    return cand[[late[0], never[0], late[1]]]


@functools.lru_cache(maxsize=None)
def rare_pose_sets():
    """name -> (poses, params): the first pose takes the rare branch (in some cycle, or in all), the second is the interior pose of
    tests/test_gpu_fast_search_edges.py and stays on the straight path, the third takes the rare branch again."""
    sets = {}
    for edge in ("top", "bottom", "left", "corner"):  # walks that reach the border (or leave it) within one batch: the flip is mid-batch
        walks, wp = border_walks(N, edge), params_of(step=SHORT, drift=RES)
        mixed = np.nonzero(mixed_batches(oracle_plan(wp, *hostile_map(N), walks, 8), N))[0]  # (which of the five starts: by the oracle)
        assert mixed.size >= 2, edge
        w = walks["position"][:, :2]
        sets["walk_" + edge] = (xyz([w[mixed[0]], INNER, w[mixed[-1]]]), wp)
    sets["magnitude"] = (xyz([(1e6, 0.0), INNER, (-1e6, 0.1)]), params_of(step=SHORT))
    sets["nan"] = (nan_centre_poses(), params_of(step=SHORT))
    sets["boundary"] = (xyz([boundary_inputs(), INNER, boundary_inputs()]), params_of(step=SHORT))
    return sets


@functools.lru_cache(maxsize=None)
def rare_inputs(name, n):
    """(trav, elev, poses, params, oracle's plan) of a rare-ballot set, with the assertion that it reaches its branch."""
    poses, params = rare_pose_sets()[name]
    trav, elev = speckled_map() if name == "nan" else hostile_map(N)
    ora = oracle_plan(params, trav, elev, poses, n)
    nom = ora["nominal"]
    inner_clear = (np.abs(ora["default"][1, :, :, :2]) < HALF - 4 * RES).all()  # every leg centre four cells and more inside the map
    if name.startswith("walk"):
        if n >= 8:
            assert mixed_batches(ora, N)[[0, 2]].all(), "both walking poses have a clear cycle and a border cycle in the first batch"
    elif name == "nan":
        if n >= 8:
            assert np.isnan(nom["x"][[0, 2]]).any(axis=(1, 2)).all() and not np.isnan(nom["x"][[0, 2], 0]).any() and not np.isnan(nom["x"][1]).any()
    elif name == "magnitude":
        assert (nom["valid"][[0, 2]] == 0).all() and (ora["centroid"]["code"][[0, 2]] == 6).all()
        assert inner_clear and nom["valid"][1].any()
    else:
        assert inner_clear
    return trav, elev, poses, params, ora


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", ["walk_top", "walk_bottom", "walk_left", "walk_corner", "magnitude", "nan", "boundary"])
def test_rare_ballot(planner, name, B, n):
    """B = 1: the rare pose alone; 2: beside the pose that stays on the straight path; 3: a second rare pose and the padding slot."""
    trav, elev, poses, params, _ = rare_inputs(name, n)
    both(planner, params, "nrl2", trav, elev, poses[:B], n)


@pytest.mark.parametrize("name", ["walk_corner", "nan", "boundary"])
def test_rare_ballot_in_the_general_copy(planner, name):
    trav, elev, poses, params, _ = rare_inputs(name, 9)
    run_general(planner, params, "nrl2", trav, elev, poses, 9)


@pytest.mark.parametrize("cls", ["nrl3", "nrl4"])
def test_rare_ballot_wider_windows(planner, cls):
    """A walk into the corner, a centre of 1e6 and a corner on a cell boundary, each beside the interior pose; and chains that reach
    a non-finite centre."""
    w = border_walks(N, "corner")["position"][:, :2]
    poses = xyz([w[2], INNER, (1e6, 0.0), INNER, boundary_inputs(cls), INNER])
    ora = both(planner, params_of(cls, step=SHORT, drift=RES), cls, *hostile_map(N), poses, 9)
    assert mixed_batches(ora, N)[0] and (ora["nominal"]["valid"][2] == 0).all()
    ora = both(planner, params_of(cls, step=SHORT), cls, *speckled_map(), nan_centre_poses(), 9)
    assert np.isnan(ora["nominal"]["x"]).any()


# ---- 2. !found && !searched: the candidate search beyond the first sixteen ranks ----------------------------------------------------
LEG = 0


@functools.lru_cache(maxsize=None)
def search_inputs(cls):
    """Three poses on good terrain but for the neighbourhood of leg 0's default cell in cycle 0: pose 0 — the 5 x 5 cells around
    it fail (every one of the first sixteen ranks), the cells beyond pass: a later rank wins; pose 1 — exactly the cell of rank 2
    passes (the straight-line search finds it); pose 2 — everything within the window's reach and two cells more fails: no
    candidate at all.  Returns (trav, elev, poses, the free cells of leg 0)."""
    params = params_of(cls)
    R = float(params["searchRadius"][0])
    js = np.array([24, 48, 72])
    off = oracle_plan(params, *synth.flat_map(N, N), xyz([(-0.2, 0.0)]), 1)["default"][0, 0, LEG, 1]
    poses = xyz([(x, Y_C[j] - off + 0.05 * RES) for x, j in zip((0.1, -0.2, -0.5), js)])
    trav, elev = synth.flat_map(N, N)
    elev += (0.001 * np.arange(N * N, dtype=np.float32).reshape(N, N) % 0.05).astype(np.float32)
    free = oracle_plan(params, trav, elev, poses, 1)["nominal"][:, 0, LEG]
    assert (free["source"] == 0).all() and (free["valid"] == 1).all()
    omap = fpo.OracleMap(trav, elev, RES)
    reach = int(np.ceil(R / RES)) + 2
    for k, (h, keep) in enumerate(((2, None), (2, 2), (reach, None))):
        ci, cj = int(free["row"][k]), int(free["col"][k])
        cells = [tuple(int(v) for v in c) for c in np.asarray(omap.spiral_cells(float(free["x"][k]), float(free["y"][k]), R))[:16]]
        assert cells[0] == (ci, cj) and all(abs(i - ci) <= 2 and abs(j - cj) <= 2 for i, j in cells)
        trav[max(ci - h, 0):ci + h + 1, max(cj - h, 0):cj + h + 1] = 0.0
        if keep is not None:
            trav[cells[keep]] = 1.0
    return trav, elev, poses, free


def assert_search_outcomes(nom0, free):
    """cycle 0, leg 0 of the three poses in the oracle's plan: rank >= 16 (three rings or more out), rank 2, none"""
    ring = max(abs(int(nom0["row"][0]) - int(free["row"][0])), abs(int(nom0["col"][0]) - int(free["col"][0])))
    assert nom0["valid"][0] == 1 and nom0["source"][0] == 1 and ring >= 3, nom0[0]
    assert nom0["valid"][1] == 1 and nom0["source"][1] == 1, nom0[1]
    assert nom0["valid"][2] == 0, nom0[2]


@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("cls", ["nrl2", "nrl3", "nrl4"])
def test_search_beyond_the_sixteen(planner, cls, n):
    trav, elev, poses, free = search_inputs(cls)
    for order in ([0, 1, 2], [2, 1], [0]):  # later rank + rank 2 / padding slot with none; none + rank 2; the later rank alone
        ora = both(planner, params_of(cls), cls, trav, elev, poses[order], n)
        if order == [0, 1, 2]:
            assert_search_outcomes(ora["nominal"][:, 0, LEG], free)
    if cls == "nrl2":
        run_general(planner, params_of(cls), cls, trav, elev, poses, n)


# ---- 3. div3's range guard --------------------------------------------------------------------------------------------------------
STEP_EXACT = 0.125  # half of it is a power of two: (+-lengthBase/2 + x0) - step/2 is exact, the shifted stance symmetric about 0


def stance_centre_x(ora, params, pose):
    """getPolygonCenter's x over the shifted stance of the oracle's plan, in the reference's expression order"""
    half = float(np.float32(params["stepLength"][0]) / np.float32(2))
    f = ora["stance"][pose].astype(np.float64).copy()
    f[:, 0] -= half
    x1, y1 = f[0, 0], f[0, 1]
    x2, y2 = f[1, 0], f[1, 1]
    sum_x = sum_s = 0.0
    for i in (1, 2):
        x3, y3 = f[i + 1, 0], f[i + 1, 1]
        s = ((x2 - x1) * (y3 - y1) - (x3 - x1) * (y2 - y1)) / 2.0
        sum_x += (x1 + x2 + x3) * s
        sum_s += s
        x2, y2 = x3, y3
    return (sum_x / sum_s) / 3.0


@functools.lru_cache(maxsize=None)
def zero_centre_inputs(cls="nrl2"):
    params = params_of(cls, step=STEP_EXACT)
    half = float(np.float32(STEP_EXACT) / np.float32(2))
    poses = xyz([(half, 0.05), INNER, (half, -0.31)])
    ora = oracle_plan(params, *speckled_map(), poses, 1)
    assert stance_centre_x(ora, params, 0) == 0.0 and stance_centre_x(ora, params, 2) == 0.0 and stance_centre_x(ora, params, 1) != 0.0
    return params, poses


@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("B", BS)
def test_div3_guard_zero_centre(planner, B, n):
    """The feet-polygon centre of the shifted stance is exactly 0.0: the first cycle's centre (and its gate's) takes the division
    itself.  (A centre at the 1e-300 scale cannot be built from a pose: the stance adds half the base length to it.  The other
    side of the guard that a chain reaches is the non-finite centre of nan_centre_poses, in test_rare_ballot.)"""
    params, poses = zero_centre_inputs()
    both(planner, params, "nrl2", *speckled_map(), poses[:B], n)


@pytest.mark.parametrize("cls", ["nrl3", "nrl4"])
def test_div3_guard_wider_windows(planner, cls):
    params, poses = zero_centre_inputs(cls)
    both(planner, params, cls, *speckled_map(), poses, 2)
    if cls == "nrl3":
        run_general(planner, params, cls, *speckled_map(), poses, 2)


# ---- 4. the !safe ballots of the y fill and of the first cycle's gate -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def y_inputs():
    """Pose 0: leg 0's y exactly on the boundary between columns 40 and 41 (drift 0: in every cycle); pose 1: the interior pose;
    pose 2: the gate's rectangle reaches over the +x edge (its gate fails by the reference's own expressions); pose 3: passes."""
    params = params_of(drift=0.0)
    off = oracle_plan(params, *synth.flat_map(N, N), xyz([(-0.2, 0.0)]), 1)["default"][0, 0, :, 1]
    boundary = Y_C[40] - 0.5 * RES
    poses = xyz([(-0.2, boundary - off[0]), INNER, (HALF - 0.02, -0.31), (0.1, 0.2)])
    ora = oracle_plan(params, *speckled_map(), poses, 2)
    assert (ora["default"][0, :, 0, 1] == boundary).all(), "leg 0's y is the boundary itself, in both cycles"
    assert ora["pose_status"].tolist() == [0, 0, _capi.FPE_POSE_OPT_SUBMAP_FAILED, 0]
    return params, poses


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("order", [[0], [0, 1], [1, 0, 2], [2, 3], [3, 1, 2]])
def test_y_fill_and_gate(planner, order, n):
    params, poses = y_inputs()
    both(planner, params, "nrl2", *speckled_map(), poses[order], n)


def test_y_fill_and_gate_general_copy_and_wider_windows(planner):
    params, poses = y_inputs()
    run_general(planner, params, "nrl2", *speckled_map(), poses, 9)
    for cls in ("nrl3", "nrl4"):
        both(planner, params_of(cls, drift=0.0), cls, *speckled_map(), poses, 2)


# ---- 5. the cycle of the priority hand-over ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_priority_handover_cycle(planner, n):
    """n * 3 / 8 is the hand-over cycle of a wavefront in an odd hardware wave slot: 0 for n = 1 and 2, 1 for n = 3, 3 for n = 8;
    none (-1) in an even slot.  4096 poses = 2048 wavefronts of the same two poses fill both slots of every SIMD: every wavefront's
    records are the first one's, and the first one's are the oracle's."""
    trav, elev = speckled_map()
    params = params_of()
    pair = xyz([(-0.45, -0.2), INNER])
    for products in (util.DEFAULT_PRODUCTS, NOMINAL_ONLY):
        check(planner, params, KERNEL["nrl2"], trav, elev, pair, n, products=products)
        eng = planner.plan(np.tile(pair, 2048), n, products=products)
        with planner.tuning(no_bits=1):
            direct = planner.plan(pair, n, products=products)
        for k, v in eng.items():
            v = np.ascontiguousarray(v).reshape((2048, -1))
            first = np.ascontiguousarray(direct[k]).reshape(-1)
            assert v.shape[1] * v.itemsize == first.size * first.itemsize, k
            assert all(row.tobytes() == first.tobytes() for row in v), f"{k}: a wavefront's records differ from the first one's"
