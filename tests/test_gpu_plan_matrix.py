"""Every bit-window kernel that launch_plan can launch, against the oracle: one table row on each side of every bits_shape switch
(window sides 15|17, 23|25, 31|33, 63|65, 95|97), every product shape on each row, odd and even batches, cycle counts on
both sides of the eight-cycle flush, the sixteen-poses-per-workgroup launch with a partly empty last workgroup, the refusal
edges of bits_supported, and exact-tie geometry (tests/tie_fixtures.py).  Each case asserts which kernel ran
(describe_plan), so a change that silently moves a configuration to another kernel fails here; the last test prints the
instantiations that ran and asserts that every one the table promises was among them."""
from collections import namedtuple

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi, synth
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner, make_poses
from tests import tie_fixtures, util

pytestmark = pytest.mark.gpu

# The window half-width (csrc/fpe_host.cpp::bits_window_halfwidth) of a radius R = q res with q = m - 0.3 (no tie) is
# m + footReach: m rows of the centroid rectangle / spiral rings, footReach rows of a candidate's foot disc.  footReach is 0
# for a one-cell disc (rf < res; with rf >= 0.9 res that is the 3x3-only MID variant), 1 for rf in (res, sqrt(2) res] and for
# 0.02 on a 1 cm map (rf just below 2 res: 9 cells), 3 for 0.02 on a 0.5 cm map (45 cells).  Parameters and names were read off
# describe_plan() once on an MI355X and are frozen here.
Row = namedtuple("Row", "id res R rf maxleg rows cols winH kernel")
MATRIX = [
    # side 15 | 17: plan_bits_kernel<2, *> | <3, *>
    Row("w7_mid", 0.02, 0.134, 0.02, None, 200, 180, 7, "plan_bits_kernel<2, true>"),
    Row("w7_gen", 0.02, 0.114, 0.03, None, 200, 180, 7, "plan_bits_kernel<2, false>"),
    Row("w8_mid", 0.02, 0.154, 0.02, None, 200, 180, 8, "plan_bits_kernel<3, true>"),
    Row("w8_gen", 0.02, 0.134, 0.03, None, 200, 180, 8, "plan_bits_kernel<3, false>"),
    # side 23 | 25: <3, *> | <4, *>
    Row("w11_mid", 0.01, 0.107, 0.0095, None, 400, 360, 11, "plan_bits_kernel<3, true>"),
    Row("w11_gen", 0.01, 0.097, 0.02, None, 400, 360, 11, "plan_bits_kernel<3, false>"),
    Row("w12_mid", 0.01, 0.117, 0.0095, None, 400, 360, 12, "plan_bits_kernel<4, true>"),
    Row("w12_gen", 0.01, 0.107, 0.02, None, 400, 360, 12, "plan_bits_kernel<4, false>"),
    # side 31 | 33: <4, *> | plan_bits_seq_kernel<1, 2> (the one-wavefront-per-pose kernels have no MID variant)
    Row("w15_mid", 0.01, 0.147, 0.0095, None, 400, 360, 15, "plan_bits_kernel<4, true>"),
    Row("w15_gen", 0.01, 0.137, 0.02, None, 400, 360, 15, "plan_bits_kernel<4, false>"),
    Row("w16_seq", 0.01, 0.137, 0.02, 0.147, 400, 360, 16, "plan_bits_seq_kernel<1, 2>"),
    # side 63 | 65: plan_bits_seq_kernel<1, 2> | <2, 3>
    Row("w31_seq", 0.005, 0.12, 0.02, 0.1385, 640, 560, 31, "plan_bits_seq_kernel<1, 2>"),
    Row("w32_seq", 0.005, 0.12, 0.02, 0.1435, 640, 560, 32, "plan_bits_seq_kernel<2, 3>"),
    # side 95 | 97: <2, 3> | no bit kernel fits: the direct one-wavefront-per-pose kernel
    Row("w47_seq", 0.005, 0.15, 0.02, 0.2185, 640, 560, 47, "plan_bits_seq_kernel<2, 3>"),
    Row("w48_direct", 0.005, 0.15, 0.02, 0.2235, 640, 560, 48, "plan_sequential_kernel (direct"),
]
ROWS = {r.id: r for r in MATRIX}

SHAPES = [util.DEFAULT_PRODUCTS, ("selected_packed",), ("nominal", "cycle_ok"), ("centroid", "stance", "selected")]
assert [util.product_shape(p) for p in SHAPES] == [2, 1, 1, 0]

# (kernel name, instantiation) -> launches, filled by every comparison below.  Instantiation: ("prod", shape) for the 8-lane
# kernels; ("kProd", 0 | 1, "GRP", 1 | 16) for the one-wavefront-per-pose kernels; () for a direct kernel.
SEEN = {}


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


def kernel_name(planner):
    return planner.describe_plan().split("(")[0].strip()


def note(planner, products, B):
    """Record the instantiation select_plan_kernel picks for this call (csrc/fpe_plan_launch.hpp)."""
    name, shape = kernel_name(planner), util.product_shape(products)
    if name.startswith("plan_bits_kernel"):
        key = (name, ("prod", shape))
    elif name.startswith("plan_bits_seq_kernel"):
        # the all-seven shape takes the generic instantiation here; sixteen poses per workgroup on 96-bit rows from 64 poses
        # (every pose slot is at most 10 KiB, so sixteen always fit the 160 KiB)
        key = (name, ("kProd", 1 if shape == 1 else 0, "GRP", 16 if name.endswith("<2, 3>") and B >= 64 else 1))
    else:
        key = (name, ())
    SEEN[key] = SEEN.get(key, 0) + 1


def row_inputs(row, B, seed, seq):
    """Map and poses of a table row: the map's border lies inside the pose range (clipped windows, centres outside), a
    quarter of the poses are lattice-aligned; the seq rows mix gaits, polygon kinds and per-leg radii."""
    rng = np.random.default_rng(seed)
    # fewer bad cells under a larger foot disc (1, 9 .. 37 or 45 cells), so that searches both succeed and fail on every row
    cells = row.rf / row.res
    bad_frac = 0.25 if cells < 1.0 else 0.07 if cells < 2.0 else 0.03 if cells < 3.5 else 0.015
    trav, elev = synth.rough_map(row.rows, row.cols, row.res, seed=seed, bad_frac=bad_frac, nan_frac=0.002, stair_period=1.1)
    lx, ly = row.rows * row.res, row.cols * row.res
    xs, ys = rng.uniform(-0.5 * lx - 0.3, 0.5 * lx - 0.4, B), rng.uniform(-0.5 * ly - 0.25, 0.5 * ly + 0.25, B)
    q = B // 4
    xs[:q], ys[:q] = np.round(xs[:q] / row.res) * row.res, np.round(ys[:q] / row.res) * row.res
    poses = make_poses(np.column_stack([xs, ys, rng.uniform(-0.1, 0.1, B)]))
    poses["gait"] = rng.integers(0, 2, B)
    if seq:
        rmax = float(row.maxleg or row.R)
        poses["leg_search_radius"] = rng.uniform(0.4 * rmax, rmax, (B, 4)).astype(np.float32)
        poses["leg_search_radius"][rng.random((B, 4)) < 0.3] = 0.0  # fpe_params.searchRadius
        poses["leg_search_radius"][0, 0] = np.float32(rmax)  # the widest window really occurs
        poses["leg_polygon_kind"] = rng.integers(0, 2, (B, 4))
    return trav, elev, poses


def configure(planner, row):
    set_params(planner, searchRadius=np.float32(row.R), footRadius=np.float32(row.rf))
    planner.set_max_leg_search_radius(float(row.maxleg or 0.0))


def check_row_name(planner, row):
    d = planner.describe_plan()
    assert d.startswith(row.kernel), (row.id, d)
    if "bit window" in d:  # the half-width the table documents, so a row stays ON its side of the switch
        side = 2 * row.winH + 1
        assert f"{side} x {side} bit window" in d, (row.id, d)


def compare(planner, poses, n, products, ora, what):
    eng = planner.plan(poses, n, products=products)
    try:
        util.assert_products_equal(eng, util.slice_plan(ora, poses.shape[0]), products)
    except AssertionError as e:
        raise AssertionError(f"{what}, B {poses.shape[0]}, n {n}, products {products}, {planner.describe_plan()}: {e}") from None
    note(planner, products, poses.shape[0])
    return eng


@pytest.mark.parametrize("row", MATRIX, ids=[r.id for r in MATRIX])
def test_matrix_row_every_product_shape(planner, row):
    """Each row: an odd batch with 7 cycles and an even batch with 9, every product shape, against the oracle."""
    seq = "seq" in row.kernel
    configure(planner, row)
    try:
        for B, n, seed in ((33, 7, 1), (48, 9, 2)):
            trav, elev, poses = row_inputs(row, B, 7000 + 10 * MATRIX.index(row) + seed, seq)
            planner.gridmapCallback(trav, elev, row.res)
            check_row_name(planner, row)
            ora = util.run_oracle(planner, trav, elev, row.res, poses, n, threads=8)
            for products in SHAPES:
                compare(planner, poses, n, products, ora, row.id)
            # the row is not idle: searches run, some fail, the centroid row scan runs, some windows are clipped by the border
            src, code = ora["nominal"]["source"], ora["centroid"]["code"]
            assert (src == 1).any() and (src == 0).any() and (ora["nominal"]["valid"] == 0).any() and (code > 0).any(), row.id
            nom = ora["nominal"]
            near_border = (nom["row"] < row.winH) | (nom["col"] < row.winH) | (nom["row"] >= row.rows - row.winH) | (nom["col"] >= row.cols - row.winH)
            assert (near_border & (nom["valid"] != 0)).any(), row.id
    finally:
        planner.set_max_leg_search_radius(0.0)


@pytest.mark.parametrize("row_id", ["w32_seq", "w47_seq"])
def test_sixteen_poses_per_workgroup_with_a_partly_empty_last_workgroup(planner, row_id):
    """plan_bits_seq_kernel<2, 3, *, 16> is launched for B >= 64 with (B + 15) / 16 workgroups of sixteen wavefronts: B = 63
    stays with one pose per workgroup, 64 fills four workgroups, 65 and 79 leave a last workgroup of 1 and 15 poses.
    One oracle plan of 79 poses serves all four (poses are independent)."""
    row = ROWS[row_id]
    configure(planner, row)
    try:
        trav, elev, poses = row_inputs(row, 79, 7500 + MATRIX.index(row), True)
        planner.gridmapCallback(trav, elev, row.res)
        check_row_name(planner, row)
        ora = util.run_oracle(planner, trav, elev, row.res, poses, 9, threads=8)
        for B in (63, 64, 65, 79):
            for products in SHAPES:
                compare(planner, poses[:B], 9, products, ora, row.id)
    finally:
        planner.set_max_leg_search_radius(0.0)


@pytest.mark.parametrize("row_id,B", [("w47_seq", 21), ("w47_seq", 66), ("w32_seq", 21), ("w16_seq", 21)])
def test_staged_record_slots_at_seventeen_cycles(planner, row_id, B):
    """recSlots, the cycles of staged records per pose (select_plan_kernel, csrc/fpe_plan_launch.hpp): 8, halved while
        base + recSlots * 4 * sizeof(SeqRec) > 10240,
        base = sizeof(PoseShared) + 4 * sizeof(LegStatic) + 4 * legbits_words(rows, KW, nHW)      (each term a multiple of 16)
             = 1664 + 288 + 4 * ((2 + max(nHW, 1)) * rows * KW rounded up to 4),    sizeof(SeqRec) = 144, rows = 2 winH + 1.
    The 0.02 m foot disc on a 0.5 cm map has the row half-widths 3, 3, 3, 2: nHW = 2, four row arrays.
      w47_seq: rows 95, KW 3: base = 1952 + 4 * 1140 = 6512; + 8 * 576 = 11120 > 10240, + 4 * 576 = 8816: recSlots = 4
      w32_seq: rows 65, KW 3: base = 1952 + 4 *  780 = 5072; + 8 * 576 =  9680:                           recSlots = 8
      w16_seq: rows 33, KW 2, nHW 1 (0.02 m on 1 cm: half-widths 1, 1): base = 1952 + 4 * 200 = 2752:   recSlots = 8
    recSlots 2 and 1 cannot occur: they need base > 7936, i.e. more than 5984 bytes of row arrays; 95 rows of 3 words take
    that with nHW >= 4 only, and four distinct half-widths need a disc of five rows or more each side, whose bounding box
    bits_supported refuses (kBitsMaxBoxCells).  Seventeen cycles = four full flushes of four slots and one partial, or two of
    eight and one partial; B = 66 runs the same through the sixteen-pose workgroups."""
    row = ROWS[row_id]
    configure(planner, row)
    try:
        trav, elev, poses = row_inputs(row, B, 7600 + MATRIX.index(row) + B, True)
        poses["position"][:, 0] -= 1.0  # seventeen cycles of 0.18 m: start further back, so that most stay on the map
        planner.gridmapCallback(trav, elev, row.res)
        check_row_name(planner, row)
        ora = util.run_oracle(planner, trav, elev, row.res, poses, 17, threads=8)
        for products in SHAPES:
            compare(planner, poses, 17, products, ora, row.id)
        assert ora["cycle_ok"][:, 16].any(), "no pose reaches the seventeenth cycle"
    finally:
        planner.set_max_leg_search_radius(0.0)


SINGLES = [(p,) for p in util.DEFAULT_PRODUCTS]
SIX_OF_SEVEN = [tuple(p for p in util.DEFAULT_PRODUCTS if p != drop) for drop in util.DEFAULT_PRODUCTS]


@pytest.mark.parametrize("row_id", ["w8_gen", "w32_seq"])
def test_every_single_product_and_every_six_of_seven(planner, row_id):
    """Fourteen subsets on an 8-lane row and a one-wavefront-per-pose row: whatever pointer is null, nothing else changes."""
    row = ROWS[row_id]
    configure(planner, row)
    try:
        trav, elev, poses = row_inputs(row, 35, 7700 + MATRIX.index(row), "seq" in row.kernel)
        planner.gridmapCallback(trav, elev, row.res)
        check_row_name(planner, row)
        ora = util.run_oracle(planner, trav, elev, row.res, poses, 9, threads=8)
        assert len(SINGLES + SIX_OF_SEVEN) == 14
        for products in SINGLES + SIX_OF_SEVEN:
            compare(planner, poses, 9, products, ora, row.id)
    finally:
        planner.set_max_leg_search_radius(0.0)


# ---- the refusal edges of bits_supported --------------------------------------------------------------------------
# (what, res, searchRadius, footRadius inside, kernel inside, footRadius outside, kernel outside)
EDGES = [
    # nFoot <= kDiscRounds * 8 = 32 on the 8-lane kernels: a^2 + b^2 < (rf / res)^2 holds for 29 lattice points at 3.1 and for 37
    # at 3.2 (the eight points (+-1, +-3), (+-3, +-1) join at sqrt(10)).  Bounding box 10 x 10 = 100 cells on both sides, within
    # legbits_words(32, 1, 3) = 160, so the box bound is not what refuses.  winH = 10 + 3.
    ("nfoot_8lane", 0.01, 0.097, 0.031, "plan_bits_kernel<4, false>", 0.032, "plan_sequential_kernel"),
    # disc bounding box (2 ceil(rf / res) + 2)^2 <= legbits_words(8 NRL, 1, nHW) = (2 + nHW) * 8 NRL on the 8-lane kernels.  NRL 2,
    # a box of 8 x 8 = 64 cells on both sides: rf = 2.5 res has the row half-widths 2, 2, 1 (nHW 2): 64 <= 4 * 16, just inside;
    # rf = 2.9 res has 2, 2, 2 (nHW 1): 64 > 3 * 16.  21 and 25 cells, so nFoot <= 32 passes on both sides.  winH = 5 + 2.
    ("box_8lane", 0.01, 0.047, 0.025, "plan_bits_kernel<2, false>", 0.029, "plan_chained_kernel<8, false>"),
    # disc bounding box <= kBitsMaxBoxCells = 128 on the 64-lane kernels: ceil(rf / res) = 4 gives 10 x 10, 5 gives 12 x 12 = 144.
    # rf = 4.1 res has 49 cells, so nFoot <= 64 passes.  The nFoot bound of the 64-lane kernels cannot refuse on its own: more
    # than 64 cells need rf > 4.5 res, whose box is already refused (and bits_window_halfwidth gives 0 above 64).
    ("box_64lane", 0.005, 0.1, 0.0195, "plan_bits_seq_kernel<1, 2>", 0.0205, "plan_sequential_kernel"),
]


@pytest.mark.parametrize("edge", EDGES, ids=[e[0] for e in EDGES])
def test_refusal_edges_of_bits_supported(planner, edge):
    what, res, R, rf_in, k_in, rf_out, k_out = edge
    rows, cols = (360, 320) if res == 0.01 else (520, 480)
    row = Row(what, res, R, rf_in, None, rows, cols, 0, k_in)
    trav, elev, poses = row_inputs(row, 41, 7800 + len(what), False)
    planner.set_max_leg_search_radius(0.0)
    for rf, kernel in ((rf_in, k_in), (rf_out, k_out)):
        set_params(planner, searchRadius=np.float32(R), footRadius=np.float32(rf))
        planner.gridmapCallback(trav, elev, res)
        assert planner.describe_plan().startswith(kernel), (what, rf, planner.describe_plan())
        ora = util.run_oracle(planner, trav, elev, res, poses, 5, threads=8)
        for products in SHAPES:
            compare(planner, poses, 5, products, ora, f"{what} rf {rf}")
        assert (ora["nominal"]["source"] == 1).any() and (ora["centroid"]["code"] > 0).any()


@pytest.mark.parametrize("row_id,group,kernel", [
    ("w8_gen", 8, "plan_bits_kernel<3, false>"),      # the 8-lane bit kernels ARE the grouping 8
    ("w8_gen", 65, "plan_sequential_kernel"),         # any other forced grouping is a request for that direct kernel
    ("w8_mid", 65, "plan_sequential_kernel"),
    ("w16_seq", 65, "plan_bits_seq_kernel<1, 2>"),    # one wavefront per pose is the grouping 65
    ("w16_seq", 8, "plan_chained_kernel<8, false>"),
    ("w32_seq", 65, "plan_bits_seq_kernel<2, 3>"),
])
def test_forced_lane_grouping_keeps_the_bit_kernel_only_where_it_is_that_grouping(planner, row_id, group, kernel):
    """bits_supported: groupOverride != 0 && groupOverride != (lanes == 8 ? 8 : 65) refuses."""
    row = ROWS[row_id]
    configure(planner, row)
    try:
        trav, elev, poses = row_inputs(row, 37, 7900 + MATRIX.index(row) + group, "seq" in row.kernel)
        planner.gridmapCallback(trav, elev, row.res)
        with planner.tuning(plan_group=group):
            assert planner.describe_plan().startswith(kernel), (row_id, group, planner.describe_plan())
            ora = util.run_oracle(planner, trav, elev, row.res, poses, 5, threads=8)
            for products in (util.DEFAULT_PRODUCTS, ("selected_packed",), ("centroid", "stance", "selected")):
                compare(planner, poses, 5, products, ora, f"{row_id} plan_group {group}")
        check_row_name(planner, row)  # and the automatic dispatch is back
    finally:
        planner.set_max_leg_search_radius(0.0)


# ---- exact ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tie_fixtures.NAMES)
def test_exact_tie_geometry(planner, name):
    """Cell centres ON the search circle, rectangle edges ON cell edges (tests/tie_fixtures.py; that the ties decide outcomes
    is proved on the oracle in tests/test_cpu_tie_fixtures.py).  The kernel name carries the window side: k + 1 rows each way
    for a radius of k cells — the tie row of bits_window_halfwidth's `reach` — where the foot disc does not reach further.
    (That row guards against rounding; with these dyadic inputs results equal the oracle without it, so the name alone pins it.)"""
    fx = tie_fixtures.make(name)
    planner.params = fx["params"]
    planner.set_max_leg_search_radius(fx["maxleg"])
    try:
        eng, ora = util.run_both(planner, fx["trav"], fx["elev"], fx["res"], fx["poses"], fx["n"], position=fx["pos"], threads=8,
                                 products=util.ALL_PRODUCTS)
        assert planner.describe_plan().startswith(fx["kernel"]), (name, planner.describe_plan())
        util.assert_plan_equal(eng, ora)
        util.assert_products_equal(eng, ora, util.ALL_PRODUCTS)
        note(planner, util.ALL_PRODUCTS, fx["poses"].shape[0])
        for products in SHAPES[1:]:
            compare(planner, fx["poses"], fx["n"], products, ora, name)
    finally:
        planner.set_max_leg_search_radius(0.0)
        set_params(planner)


# ---- what ran -----------------------------------------------------------------------------------------------------
def promised():
    """Every plain-form instantiation visit_lane8 / visit_seq name (csrc/fpe_plan_launch.hpp) — 18 of plan_bits_kernel<NRL, MID, PROD>,
    6 of plan_bits_seq_kernel<NRL, KW, kProd, GRP> — and the direct kernels on the far side of the refusal edges."""
    want = {(f"plan_bits_kernel<{nrl}, {mid}>", ("prod", s)) for nrl in (2, 3, 4) for mid in ("true", "false") for s in (0, 1, 2)}
    want |= {("plan_bits_seq_kernel<1, 2>", ("kProd", k, "GRP", 1)) for k in (0, 1)}  # GRP 16 is for KW >= 3 only:
    want |= {("plan_bits_seq_kernel<2, 3>", ("kProd", k, "GRP", g)) for k in (0, 1) for g in (1, 16)}  # <1, 2, *, 16> is not compiled
    want |= {("plan_sequential_kernel", ()), ("plan_chained_kernel<8, false>", ())}
    return want


def test_zz_every_promised_instantiation_ran():
    """Last in the module (run the module as a whole): the kernels exercised, with their product shapes."""
    for (name, inst), count in sorted(SEEN.items()):
        print(f"plan matrix coverage: {name} {' '.join(map(str, inst))}: {count} comparisons with the oracle")
    print("plan matrix coverage:", len([k for k in SEEN if k[0].startswith("plan_bits_kernel")]), "of 18 plan_bits_kernel and",
          len([k for k in SEEN if k[0].startswith("plan_bits_seq_kernel")]), "of 6 launchable plan_bits_seq_kernel instantiations; direct:",
          sorted({k[0] for k in SEEN if not k[0].startswith("plan_bits")}))
    missing = promised() - set(SEEN)
    assert not missing, f"never ran: {sorted(missing)}"
