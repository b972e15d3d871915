"""The 8-lane, two-poses-per-wavefront plan kernel (3x3-only variant, every product written: bench.py's headline launch) on
the shapes its fast paths branch on: a last wavefront holding one pose, a batch of one, cycle counts on both sides of the
eight-cycle flush, maps where the 16-candidate search runs in every cycle and in none, and windows clipped by the map border.
Bar: the suite's own (tests/util.py): indices / flags / x / y bit-exact against the oracle, |dz| <= 1e-6."""
import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi, synth
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_poses
from tests import util

pytestmark = pytest.mark.gpu

RES = 0.02  # foot radius 0.02 at 2 cm: 3x3 disc boxes, the variant the headline launches


@pytest.fixture(scope="module")
def planner():
    p = FootholdPlanner(0)
    p.params = _capi.params_yaml()
    yield p
    p.close()


def rough(rows=300, seed=701, **kw):
    return synth.rough_map(rows, rows, RES, seed=seed, **kw)


@pytest.mark.parametrize("B", [1, 3, 33, 255])
def test_odd_batches_and_a_batch_of_one(planner, B):
    """Odd B: the last wavefront's second pose slot is padding (it runs the chain on pose B-1 and stores nothing)."""
    trav, elev = rough(bad_frac=0.15)
    poses = synth.poses_in_map(B, 6.0, 6.0, 8, 0.18, seed=710 + B, margin=0.7)
    eng, ora = util.run_both(planner, trav, elev, RES, poses, 8, threads=8)
    util.assert_plan_equal(eng, ora)
    assert eng["nominal"].shape[0] == B


@pytest.mark.parametrize("n_cycles", [1, 7, 8, 9, 17])
def test_cycle_counts_around_the_flush_boundary(planner, n_cycles):
    """Units and y entries are staged for eight cycles and flushed together: one flush short, exact, one and two flushes
    with a remainder.  Even and odd batches."""
    side = max(6.0, 0.18 * n_cycles + 3.0)
    rows = int(round(side / RES))
    trav, elev = rough(rows=rows, seed=720, bad_frac=0.15)
    for B in (64, 37):
        poses = synth.poses_in_map(B, side, side, n_cycles, 0.18, seed=730 + n_cycles + B, margin=0.7)
        eng, ora = util.run_both(planner, trav, elev, RES, poses, n_cycles, threads=8)
        util.assert_plan_equal(eng, ora)
        assert eng["nominal"].shape[:2] == (B, n_cycles)


def test_every_default_disc_fails_and_no_candidate_passes(planner):
    """No cell reaches either threshold and none is unknown: every leg's default check fails, the search runs in every
    cycle and finds nothing."""
    trav, elev = rough(seed=740, nan_frac=0.0)
    trav = np.full_like(trav, 0.1)
    poses = synth.poses_in_map(65, 6.0, 6.0, 8, 0.18, seed=741, margin=0.7)
    eng, ora = util.run_both(planner, trav, elev, RES, poses, 8, threads=8)
    util.assert_plan_equal(eng, ora)
    assert not ora["nominal"]["valid"].any() and not ora["cycle_ok"].any()


@pytest.mark.parametrize("unknown_cells", [False, True])
def test_every_default_disc_fails_and_the_search_finds_cells(planner, unknown_cells):
    """Every known cell lies between candidateFootholdThreshold (0.7) and defaultFootholdThreshold (0.9), or below both with
    unknown (NaN) cells sprinkled in: no default disc passes, the search runs in every cycle and some searches succeed."""
    trav, elev = rough(seed=750, nan_frac=0.005 if unknown_cells else 0.0)
    trav = np.where(np.isnan(trav), trav, np.float32(0.1 if unknown_cells else 0.8))
    poses = synth.poses_in_map(129, 6.0, 6.0, 8, 0.18, seed=751, margin=0.7)
    eng, ora = util.run_both(planner, trav, elev, RES, poses, 8, threads=8)
    util.assert_plan_equal(eng, ora)
    src, valid = ora["nominal"]["source"], ora["nominal"]["valid"]
    assert (src != 0).all(), "no default foothold may be accepted"
    assert ((src == 1) & (valid == 1)).any(), "some searches must succeed"


def test_no_default_disc_fails(planner):
    """Every cell traversable: the search is never entered."""
    elev = rough(seed=760, nan_frac=0.0, bad_frac=0.0)[1]
    trav = np.ones_like(elev)
    poses = synth.poses_in_map(66, 6.0, 6.0, 8, 0.18, seed=761, margin=0.7)
    eng, ora = util.run_both(planner, trav, elev, RES, poses, 8, threads=8)
    util.assert_plan_equal(eng, ora)
    assert (ora["nominal"]["source"] == 0).all() and ora["nominal"]["valid"].all() and ora["cycle_ok"].all()


@pytest.mark.parametrize("n_cycles", [3, 9])
def test_windows_clipped_by_the_map_border(planner, n_cycles):
    """Poses along all four edges of a 4 x 4 m map, from a window's reach inside it to just outside: the bit window, the
    centroid rectangle and the search rectangle are clipped, some legs leave the map."""
    trav, elev = rough(rows=200, seed=770, bad_frac=0.15)
    rng = np.random.default_rng(771)
    n = 60
    along = rng.uniform(-2.3, 2.3, size=(4, n))
    off = rng.uniform(1.55, 2.15, size=(4, n))
    xy = np.concatenate([np.stack([off[0], along[0]], 1), np.stack([-off[1] - 0.18 * n_cycles * rng.uniform(0, 1, n), along[1]], 1),
                         np.stack([along[2], off[2]], 1), np.stack([along[3], -off[3]], 1)])
    poses = make_poses(np.column_stack([xy, np.zeros(len(xy))]))[:-1]  # odd batch
    eng, ora = util.run_both(planner, trav, elev, RES, poses, n_cycles, threads=8)
    util.assert_plan_equal(eng, ora)
    assert (ora["centroid"]["code"] == 6).any() and (ora["nominal"]["valid"] == 1).any(), "poses must straddle the border"
