"""The heights of the 3x3-only 8-lane kernels from deposit to flush, and the loop nest around them (csrc/fpe_bits_lane8.hpp).
The cycle loop is a nest by batch of eight cycles (y fill, the batch's cycles, flush_unit); leg_fast8m loads the elevations of its
two 3x3 disc boxes a box ROW per lane (12-byte loads, lanes 6 and 7 repeating lanes 4 and 5) in the instances with two and three
window rows per lane and a cell per lane in the one with four; on its rare path leg_phase_bits8 deposits them; flush_unit runs the
ordered height sums.  (Loading the elevations in flush_unit instead — the chain depositing box origins only — was built and
measured slower: profiles/headline_deferred_ab_6c1b01b.txt.  These tests were written for that form and hold for either.)
What can go wrong: a batch boundary (the last batch shorter than eight, the padding slot of an odd pose count, one cycle), a
product shape without the default-track disc, elevations the height rules treat specially (NaN, +-inf, >= 10) in every slot of a
row, discs that visit only some of their nine cells, the centroid result's own cell, and batches whose units come from both
depositors (a chain that walks to the map's border).
Maps of 96 x 96 and 128 x 128 cells at 2 cm.  Every case: against the oracle (tests/util.py: indices / flags / x / y bit-exact,
|dz| <= 1e-6) and byte for byte against the direct kernels (no_bits = 1) on the same inputs.  What the inputs must contain is
asserted on the oracle's plan."""
import functools

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import synth
from quadrupedal_foothold_planner_amd.planner import make_poses

from tests import util
from tests.test_gpu_fast_search_edges import CLASSES, RES, check, class_params, oracle_plan

pytestmark = pytest.mark.gpu

# all seven products; the nominal track only (the kernels compiled without the default-track disc); the 8-byte exchange record
# alone (the same kernels, no nominal record either); and a mix that takes the any-combination kernels with no default track
PRODUCT_SETS = {"all": util.DEFAULT_PRODUCTS, "nominal_only": ("nominal", "selected", "cycle_ok"), "packed_only": ("selected_packed",),
                "mixed": ("centroid", "stance", "selected")}
assert [util.product_shape(PRODUCT_SETS[k]) for k in ("all", "nominal_only", "packed_only", "mixed")] == [2, 1, 1, 0]
KERNEL = CLASSES["nrl2"][1]


@pytest.fixture(scope="module")
def planner():
    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner

    p = FootholdPlanner(0)
    yield p
    p.set_max_leg_search_radius(0.0)
    p.set_tuning(no_bits=0)
    p.close()


def params_for(cls="nrl2", step=None, drift=None, foot=None):
    p = class_params(cls)
    if step is not None:
        p["stepLength"] = np.float32(step)
    if drift is not None:
        p["lateralDrift"] = drift
    if foot is not None:
        p["footRadius"] = np.float32(foot)
    return p


@functools.lru_cache(maxsize=None)
def hostile_map(n):
    """Traversability: four fifths pass, 12 % fail the default test only, 8 % fail both — default hits, candidate searches and
    every centroid case occur, and few cycles fail (a failed cycle commits nothing: the chain would stand still); a band
    of seventeen rows across the middle passes everywhere, so that whole centroid regions are valid there.  Elevation: uniform in +-5 cm
    with 4 % NaN, 2 % +inf, 2 % -inf and 6 % values of 10 and more (10 exactly, 12.5, 1e3), independent of the traversability:
    most discs hold a cell the height rules treat specially."""
    rng = np.random.default_rng(4711 + n)
    trav = rng.choice(np.array([1.0, 0.8, 0.5], np.float32), size=(n, n), p=[0.8, 0.12, 0.08])
    trav[n // 2 - 8:n // 2 + 9] = np.float32(1.0)
    elev = rng.uniform(-0.05, 0.05, size=(n, n)).astype(np.float32)
    kind = rng.choice(7, size=(n, n), p=[0.86, 0.04, 0.02, 0.02, 0.02, 0.02, 0.02])
    for k, v in ((1, np.nan), (2, np.inf), (3, -np.inf), (4, 10.0), (5, 12.5), (6, 1e3)):
        elev[kind == k] = np.float32(v)
    return trav, elev


def interior_poses(n_map, B):
    """Poses whose first cycles lie well inside the map, two cells apart in y from pose to pose."""
    half = 0.5 * n_map * RES
    k = np.arange(B)
    return make_poses(np.column_stack([np.full(B, -half + 0.55) + 0.013 * k, 0.031 + 2 * RES * k - 0.2, np.zeros(B)]))


def special_cells_in_discs(ora, elev):
    """Over the default hits of the oracle's plan: whether some centre disc's 3x3 box holds a NaN, an infinite and a >= 10 cell."""
    nom = ora["nominal"]
    hit = (nom["valid"] == 1) & (nom["source"] == 0)
    n = elev.shape[0]
    hit &= (nom["row"] >= 1) & (nom["row"] <= n - 2) & (nom["col"] >= 1) & (nom["col"] <= n - 2)
    got = [False, False, False]
    for r, c in zip(nom["row"][hit], nom["col"][hit]):
        box = elev[r - 1:r + 2, c - 1:c + 2]
        got[0] |= bool(np.isnan(box).any())
        got[1] |= bool(np.isinf(box).any())
        got[2] |= bool((box[np.isfinite(box)] >= 10).any())
    return got


# ---- 1. batch boundaries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17])
def test_batch_boundaries(planner, n, B):
    """Cycle counts on both sides of one and two flushes, with one pose and an empty slot, a full wavefront, and the padding slot
    of an odd batch; n = 1 puts the priority mark (n * 3 / 8) at cycle 0.  Short steps keep seventeen cycles inside the map."""
    trav, elev = hostile_map(128)
    params = params_for(step=0.08)
    poses = interior_poses(128, B)
    eng, ora = check(planner, params, KERNEL, trav, elev, poses, n)
    assert ora["cycle_ok"].shape == (B, n)
    if n >= 8:
        last = ora["nominal"][:, -1]
        assert (last["row"] >= 2).all() and (last["row"] <= 125).all(), "the last cycle is still inside the map"
        assert ora["cycle_ok"][:, n - 1].any() or ora["nominal"]["valid"][:, n - 1].any()


# ---- 2. product shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("products", list(PRODUCT_SETS))
@pytest.mark.parametrize("n", [3, 9])
def test_product_shapes(planner, products, n):
    """Each compiled product shape, with and without the default-track disc's rows and the centroid result's cell among the loads."""
    trav, elev = hostile_map(96)
    poses = interior_poses(96, 5)
    check(planner, params_for(), KERNEL, trav, elev, poses, n, products=PRODUCT_SETS[products])


# ---- 3. elevations through the row loads ----------------------------------------------------------------------------------------
def test_special_elevations_in_the_discs(planner):
    """NaN, +-inf and values >= 10 inside centre discs that hit, and centroid results (codes 1-4) whose own cell has another
    height than the leg's centre disc."""
    trav, elev = hostile_map(96)
    poses = interior_poses(96, 12)
    eng, ora = check(planner, params_for(), KERNEL, trav, elev, poses, 8)
    assert special_cells_in_discs(ora, elev) == [True, True, True]
    codes = ora["centroid"]["code"]
    for c in (1, 2, 3, 4):
        assert (codes == c).any(), f"no centroid result of code {c}"
    own = (codes >= 1) & (codes <= 4)
    assert (ora["centroid"]["z"][own] != ora["nominal"]["z"][own]).any(), "a centroid cell's height that is not the centre disc's"
    assert (codes == 0).any() and (ora["nominal"]["source"] == 1).any()


def test_partly_visited_discs(planner):
    """A foot radius of 0.91 cells: the 3x3 box stays, but a disc visits two to five of its nine cells, depending on where in
    its cell the centre lies.  Counted here from the default track's positions, which are disc centres."""
    n_map, rf = 96, 0.91 * RES
    trav, elev = hostile_map(n_map)
    params = params_for(foot=rf)
    poses = interior_poses(n_map, 12)
    eng, ora = check(planner, params, KERNEL, trav, elev, poses, 8)
    check(planner, params, KERNEL, trav, elev, poses, 8, products=PRODUCT_SETS["nominal_only"])
    xc, yc = synth.cell_centres(n_map, n_map, RES)
    d = ora["default"].reshape(-1, 3)
    counts = set()
    for x, y in d[:, :2]:
        i, j = int(np.argmin(np.abs(xc - x))), int(np.argmin(np.abs(yc - y)))
        if 1 <= i <= n_map - 2 and 1 <= j <= n_map - 2:
            dx, dy = xc[i - 1:i + 2] - x, yc[j - 1:j + 2] - y
            counts.add(int(((dx[:, None] ** 2 + dy[None, :] ** 2) <= float(np.float32(rf)) ** 2).sum()))
    assert max(counts) < 9 and len(counts) >= 3, counts


# ---- 4. fast and rare cycles in one batch -------------------------------------------------------------------------------------
def border_walks(n_map, edge):
    """Chains of eight cycles, one cell a cycle in y (the drift) and three in x (the step), that start inside the map and end at
    the named edge or corner — or, for the rear edge, start there and walk inside: the start is shifted cell by cell over five
    poses, so that some pose has a leg within two cells of the edge while its first (last) cycles are clear of it."""
    half = 0.5 * n_map * RES
    shifts = RES * np.arange(5)
    far_x, far_y = half - 0.35 - 7 * 0.06, half - 0.09 - 0.0875 - 7 * RES
    xy = {"top": [(far_x + s, 0.1) for s in shifts], "bottom": [(-half + 0.29 - s, -0.1) for s in shifts],
          "left": [(-0.3, far_y + s) for s in shifts], "right": [(-0.3, -(far_y + s)) for s in shifts],
          "corner": [(far_x + s, far_y + s) for s in shifts]}[edge]
    return make_poses(np.column_stack([np.array(xy), np.zeros(len(xy))]))


def mixed_batches(ora, n_map):
    """Poses of the oracle's plan with a cycle whose four search centres all lie three or more cells inside the map and a cycle
    with a centre within two cells of an edge (or a leg without a cell at all)."""
    nom = ora["nominal"]
    near = (nom["row"] <= 2) | (nom["row"] >= n_map - 3) | (nom["col"] <= 2) | (nom["col"] >= n_map - 3)
    clear = (~near).all(axis=2)
    return clear.any(axis=1) & near.any(axis=2).any(axis=1)


@pytest.mark.parametrize("edge", ["top", "bottom", "left", "right", "corner"])
def test_walk_to_the_border(planner, edge):
    """The first eight cycles are one batch: some of its units are deposited by the straight-line leg search, some by the general
    one (a box at the map's border, a centre outside).  All products and the nominal track alone."""
    n_map = 96
    trav, elev = hostile_map(n_map)
    params = params_for(step=0.06, drift={"right": -RES}.get(edge, RES))
    poses = border_walks(n_map, edge)
    eng, ora = check(planner, params, KERNEL, trav, elev, poses, 9)
    assert mixed_batches(ora, n_map).sum() >= 2, "chains that reach the border within a batch"
    check(planner, params, KERNEL, trav, elev, poses, 9, ora=ora, products=PRODUCT_SETS["nominal_only"])


def test_walk_to_the_border_in_the_general_copy(planner):
    """The same walks beside a walk-gait pose and a pose that overrides one leg's search radius: the wavefront takes the general
    copy of the body, whose units come from the same two depositors."""
    n_map = 96
    trav, elev = hostile_map(n_map)
    params = params_for(step=0.06, drift=RES)
    poses = np.concatenate([border_walks(n_map, "corner")[:4], border_walks(n_map, "top")[:2]])
    poses["gait"][[1, 2]] = 1
    poses["leg_search_radius"][5, 2] = np.float32(0.08)
    try:
        planner.set_max_leg_search_radius(0.09)
        eng, ora = check(planner, params, KERNEL, trav, elev, poses, 9)
    finally:
        planner.set_max_leg_search_radius(0.0)
    assert mixed_batches(ora, n_map)[[0, 3, 4]].any()


# ---- 5. three and four window rows per lane ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["nrl3", "nrl4"])
def test_wider_windows(planner, cls):
    """One case each for the instances with 17 x 17 and 25 x 25 windows: a flush and a second, short batch; special elevations."""
    trav, elev = hostile_map(96)
    poses = interior_poses(96, 5)
    eng, ora = check(planner, params_for(cls), CLASSES[cls][1], trav, elev, poses, 9)
    assert special_cells_in_discs(ora, elev) == [True, True, True]
    check(planner, params_for(cls), CLASSES[cls][1], trav, elev, poses, 9, ora=ora, products=PRODUCT_SETS["nominal_only"])
