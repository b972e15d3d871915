"""Trunk checks without a GPU: the numpy reference (tests/trunk_reference.py) against hand-computed cases on a dyadic geometry, the
refusal rules, the documented struct sizes, the defaults, and the derivation of a plan's stances from its products."""
import ctypes as C
import itertools

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi
from quadrupedal_foothold_planner_amd.planner import make_trunk_limits, make_trunk_queries
from tests import trunk_reference as ref

RES, N = 0.25, 16  # a 16 x 16 map at 0.25 m about the origin: every cell centre (1.875 - 0.25 i) and every value below is exact
INF = np.inf


def grid(elev=None):
    return ref.Grid(np.zeros((N, N), np.float32) if elev is None else np.asarray(elev, np.float32), RES)


def stance(g, i_front, i_hind, j_left, j_right, z=(0.0, 0.0, 0.0, 0.0)):
    """Feet RF, RH, LH, LF on cell centres: the front feet in row i_front (the larger x), the left feet in column j_left (the larger y)"""
    x, y = g.px[:, 0], g.py[0, :]
    return [(x[i_front], y[j_right], z[0]), (x[i_hind], y[j_right], z[1]), (x[i_hind], y[j_left], z[2]), (x[i_front], y[j_left], z[3])]


def test_box_edges_on_cell_centres_are_members():
    """Centre on cell (6, 7), hx = two cells and hy = one cell exactly: the members at distance exactly hx and hy are in — 5 x 3 cells;
    `<` would give 3 x 1."""
    g = grid()
    feet = stance(g, 4, 8, 5, 9)
    cx, cy, hx, hy, sx, sy, bz, deg = ref.frame(feet, 0.5, 0.25)
    assert (cx, cy, hx, hy, sx, sy, bz, deg) == (g.px[6, 0], g.py[0, 7], 0.5, 0.25, 0.0, 0.0, 0.0, False)
    member, ii, jj, gap = ref.members_and_gaps(g, feet, 0.5, 0.25)
    assert sorted(set(ii.tolist())) == [4, 5, 6, 7, 8] and sorted(set(jj.tolist())) == [6, 7, 8] and member.sum() == 15
    rec = ref.stance_record(g, feet, 0.5, 0.25)
    assert (rec["n_cells"], rec["n_unknown"], rec["flags"], rec["clearance"], rec["row"], rec["col"]) == (15, 0, ref.STANCE, 0.0, 4, 6)
    # one ulp less and the rim is out
    assert ref.stance_record(g, feet, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.25), np.float32(0)))["n_cells"] == 3


def test_tilted_stance_every_gap_written_out():
    """Front feet 0.5 above the hind feet over 1 m, left feet 0.25 below the right feet over 1 m: slope_x = 0.5, slope_y = -0.25;
    the feet's mean height 0.625 plus a ride height of 0.125; flat ground at 0.25."""
    g = grid(np.full((N, N), 0.25, np.float32))
    feet = stance(g, 4, 8, 5, 9, z=(1.0, 0.5, 0.25, 0.75))
    lim = make_trunk_limits(ride_height=0.125)
    cx, cy, hx, hy, sx, sy, bz, deg = ref.frame(feet, 0.25, 0.25, lim)
    assert (sx, sy, bz, deg) == (0.5, -0.25, 0.75, False)
    member, ii, jj, gap = ref.members_and_gaps(g, feet, 0.25, 0.25, lim)
    want = {(5, 6): 0.5625, (5, 7): 0.625, (5, 8): 0.6875,   # row 5 lies 0.25 m ahead of the centre: + 0.125; column 6 0.25 m to the
            (6, 6): 0.4375, (6, 7): 0.5, (6, 8): 0.5625,     # left: - 0.0625
            (7, 6): 0.3125, (7, 7): 0.375, (7, 8): 0.4375}
    assert dict(zip(zip(ii.tolist(), jj.tolist()), gap.tolist())) == want
    rec = ref.stance_record(g, feet, 0.25, 0.25, lim)
    assert (rec["clearance"], rec["row"], rec["col"], rec["slope_x"], rec["slope_y"], rec["base_z"]) == (0.3125, 7, 6, 0.5, -0.25, 0.75)
    assert rec["max_elevation"] == np.float32(0.25) and rec["flags"] == ref.STANCE
    # the limits: strict comparisons, each on its own
    flags = lambda **kw: int(ref.stance_record(g, feet, 0.25, 0.25, make_trunk_limits(ride_height=0.125, **kw))["flags"])
    assert flags(min_clearance=0.3125) == ref.STANCE and flags(min_clearance=0.3126) == ref.STANCE | ref.UNDER_CLEARANCE
    assert flags(max_slope_x=0.5, max_slope_y=0.25) == ref.STANCE
    assert flags(max_slope_x=0.49) == ref.STANCE | ref.OVER_SLOPE and flags(max_slope_y=0.2) == ref.STANCE | ref.OVER_SLOPE


def test_tie_rule_lowest_row_then_lowest_column():
    elev = np.zeros((N, N), np.float32)
    g = grid(elev)
    feet = stance(g, 4, 8, 5, 9, z=(0.5,) * 4)
    rec = ref.stance_record(g, feet, 0.25, 0.25)            # nine equal gaps
    assert (rec["clearance"], rec["row"], rec["col"]) == (0.5, 5, 6)
    elev[7, 6] = elev[6, 8] = 0.25                          # two equal minima: the lower row wins, whatever its column
    rec = ref.stance_record(grid(elev), feet, 0.25, 0.25)
    assert (rec["clearance"], rec["row"], rec["col"], rec["max_elevation"]) == (0.25, 6, 8, np.float32(0.25))
    elev[6, 7] = 0.25                                       # ... and within a row the lower column
    assert tuple(ref.stance_record(grid(elev), feet, 0.25, 0.25)[["row", "col"]].tolist()) == (6, 7)


def test_total_order_minus_zero_ranks_below_plus_zero():
    """Feet and ride height at -0.0 on ground at +0.0: base_z = -0.0, both slopes +0.0, and the slope terms sum to -0.0 only where both
    offsets are negative — cell (7, 8) — so that gap_c = -0.0 - 0.0 = -0.0 there and +0.0 in the eight other members."""
    g = grid()
    feet = stance(g, 4, 8, 5, 9, z=(-0.0,) * 4)
    lim = make_trunk_limits(ride_height=-0.0)
    _, ii, jj, gap = ref.members_and_gaps(g, feet, 0.25, 0.25, lim)
    assert [(i, j) for i, j, v in zip(ii.tolist(), jj.tolist(), gap) if np.signbit(v)] == [(7, 8)] and np.all(gap == 0.0)
    rec = ref.stance_record(g, feet, 0.25, 0.25, lim)
    assert (rec["row"], rec["col"]) == (7, 8) and rec["clearance"] == 0.0 and np.signbit(rec["clearance"]) and np.signbit(rec["base_z"])
    # max_elevation: +0.0 ranks above -0.0
    elev = np.full((N, N), -0.0, np.float32)
    assert np.signbit(ref.stance_record(grid(elev), feet, 0.25, 0.25)["max_elevation"])
    elev[6, 8] = 0.0
    assert not np.signbit(ref.stance_record(grid(elev), feet, 0.25, 0.25)["max_elevation"])


def test_no_known_member_and_the_known_cut():
    elev = np.zeros((N, N), np.float32)
    elev[5:8, 6:9] = [[np.nan, np.inf, -np.inf], [10.0, 12.0, np.nan], [np.inf, 10.0, np.nan]]
    feet = stance(grid(), 4, 8, 5, 9, z=(0.5,) * 4)
    rec = ref.stance_record(grid(elev), feet, 0.25, 0.25)
    assert (rec["clearance"], rec["row"], rec["col"], rec["n_cells"], rec["n_unknown"], rec["max_elevation"]) == (INF, -1, -1, 9, 9, 0.0)
    assert rec["flags"] == ref.STANCE | ref.UNKNOWN
    assert rec["flags"] == ref.stance_record(grid(elev), feet, 0.25, 0.25, make_trunk_limits(min_clearance=1e300))["flags"]  # inf is not under
    elev[7, 7] = np.nextafter(np.float32(10.0), np.float32(0.0))  # e < 10 is known, 10 is not
    rec = ref.stance_record(grid(elev), feet, 0.25, 0.25)
    assert (rec["row"], rec["col"], rec["n_unknown"], rec["clearance"]) == (7, 7, 8, 0.5 - np.float64(elev[7, 7]))


def test_box_on_a_cell_corner_below_half_a_cell_is_empty():
    g = grid()
    feet = stance(g, 4, 7, 5, 8)  # the centre lies on the corner shared by cells (5, 6), (5, 7), (6, 6), (6, 7)
    assert ref.frame(feet, 0.1, 0.1)[:2] == (g.px[5, 0] - 0.125, g.py[0, 6] - 0.125)
    rec = ref.stance_record(g, feet, 0.1, 0.1)
    assert (rec["n_cells"], rec["flags"], rec["clearance"], rec["row"], rec["col"]) == (0, ref.STANCE | ref.EMPTY, INF, -1, -1)
    assert ref.stance_record(g, feet, 0.125, 0.125)["n_cells"] == 4  # half a cell exactly reaches the four centres


def test_degenerate_stances_have_zero_slope_on_that_axis():
    g = grid()
    z = (1.0, 0.5, 0.25, 0.75)
    rec = ref.stance_record(g, stance(g, 6, 6, 5, 9, z), 0.25, 0.25)      # front and hind feet coincide in x
    assert (rec["slope_x"], rec["slope_y"], rec["flags"]) == (0.0, -0.25, ref.STANCE | ref.DEGENERATE)
    rec = ref.stance_record(g, stance(g, 4, 8, 7, 7, z), 0.25, 0.25)      # left and right feet coincide in y
    assert (rec["slope_x"], rec["slope_y"], rec["flags"]) == (0.5, 0.0, ref.STANCE | ref.DEGENERATE)
    rec = ref.stance_record(g, stance(g, 8, 4, 9, 5, z), 0.25, 0.25)      # crossed feet: dxf, dyl < 0
    assert (rec["slope_x"], rec["slope_y"], rec["flags"]) == (0.0, 0.0, ref.STANCE | ref.DEGENERATE)
    assert ref.stance_record(g, stance(g, 4, 8, 5, 9, z), 0.25, 0.25)["flags"] == ref.STANCE


def test_off_map_on_each_of_the_four_corners():
    """The map spans (-2, 2] on both axes (checkIfPositionWithinMap: 0 <= 2 - x < 4)."""
    g = grid()
    inside = stance(g, 4, 8, 5, 9)
    assert ref.stance_record(g, inside, 0.5, 0.5)["flags"] == ref.STANCE
    for feet, hx, hy in ((stance(g, 0, 2, 5, 9), 0.5, 0.25),     # cx = 1.625: cx + hx = 2.125 > 2
                         (stance(g, 13, 15, 5, 9), 0.5, 0.25),   # cx = -1.625: cx - hx = -2.125
                         (stance(g, 4, 8, 0, 2), 0.25, 0.5),     # cy + hy = 2.125
                         (stance(g, 4, 8, 13, 15), 0.25, 0.5)):  # cy - hy = -2.125
        rec = ref.stance_record(g, feet, hx, hy)
        assert rec["flags"] == ref.STANCE | ref.OFF_MAP and rec["n_cells"] > 0
    # the edge itself: x = 2 is on the map, x = -2 is not
    assert ref.stance_record(g, stance(g, 0, 2, 5, 9), 0.375, 0.25)["flags"] == ref.STANCE
    assert ref.stance_record(g, stance(g, 13, 15, 5, 9), 0.375, 0.25)["flags"] == ref.STANCE | ref.OFF_MAP
    far = [(x + 100.0, y, z) for x, y, z in inside]
    assert ref.stance_record(g, far, 0.5, 0.5)["flags"] == ref.STANCE | ref.OFF_MAP | ref.EMPTY


def test_refused_stances():
    g = grid()
    good = np.array(stance(g, 4, 8, 5, 9))
    assert ref.stance_record(g, good, 0.25, 0.25)["flags"] == ref.STANCE
    for leg, c, v in ((0, 0, np.nan), (1, 1, np.inf), (2, 2, -np.inf), (3, 0, 1e6 + 1.0), (0, 2, -2e6)):
        bad = good.copy()
        bad[leg, c] = v
        rec = ref.stance_record(g, bad, 0.25, 0.25)
        assert rec["flags"] == ref.REFUSED and rec.tobytes() == bytes(52) + b"\x80" + bytes(3)
    edge = good.copy()
    edge[0, 2] = 1e6  # the bound itself is a coordinate
    assert ref.stance_record(g, edge, 0.25, 0.25)["flags"] & ref.STANCE
    for hl, hw in ((np.nan, 0.25), (0.25, np.inf), (-np.inf, 0.25), (np.float32(1.0000001), 0.25), (0.25, 1.5)):
        assert ref.stance_record(g, good, hl, hw)["flags"] == ref.REFUSED
    assert ref.stance_record(g, good, 1.0, 1.0)["flags"] & ref.STANCE   # the bound itself is a half extent
    assert ref.stance_record(g, good, -1.0, 0.0)["flags"] & ref.STANCE  # <= 0: the default
    # a slope beyond +-1e6 (feet a hair apart): refused, so that no gap is ever NaN
    steep = good.copy()
    steep[[0, 3], 0] = steep[1, 0] + 1e-7
    steep[[0, 3], 2] = 1.0
    assert ref.frame(steep, 0.25, 0.25)[4] > 1e6 and ref.stance_record(g, steep, 0.25, 0.25)["flags"] == ref.REFUSED
    steep[[0, 3], 2] = 0.05
    assert 0 < ref.frame(steep, 0.25, 0.25)[4] < 1e6 and ref.stance_record(g, steep, 0.25, 0.25)["flags"] == ref.STANCE


def test_cell_cap_expression():
    """(2 hx / res + 3) (2 hy / res + 3) > 65536, in f64: at 1/256 m, 253/512 m gives 256 * 256 — the cap itself, not over."""
    res = 1.0 / 256.0
    assert not ref.box_over_cap(253.0 / 512.0, 253.0 / 512.0, res) and ref.box_over_cap(254.0 / 512.0, 253.0 / 512.0, res)
    assert ref.box_over_cap(1.0, 1.0, 0.005) and not ref.box_over_cap(1.0, 1.0, 0.02) and not ref.box_over_cap(0.22, 0.0875, 0.005)
    fine = ref.Grid(np.zeros((8, 8), np.float32), res)
    feet = stance(fine, 2, 5, 2, 5)
    assert ref.stance_record(fine, feet, 253.0 / 512.0, 253.0 / 512.0)["flags"] & ref.STANCE
    assert ref.stance_record(fine, feet, 254.0 / 512.0, 253.0 / 512.0)["flags"] == ref.REFUSED
    assert ref.stance_record(fine, feet, 0.0, 0.0, make_trunk_limits(half_length=0.5, half_width=0.5))["flags"] == ref.REFUSED


def test_limits_refusals_and_half_extent_resolution():
    assert not ref.limits_refused(None) and not ref.limits_refused(make_trunk_limits(min_clearance=INF, max_slope_x=0.0, ride_height=-1e6))
    for kw in (dict(min_clearance=np.nan), dict(max_slope_x=np.nan), dict(max_slope_y=np.nan), dict(ride_height=np.nan),
               dict(ride_height=INF), dict(ride_height=1e6 + 1.0), dict(half_length=np.nan), dict(half_width=1.0000001),
               dict(half_length=INF)):
        assert ref.limits_refused(make_trunk_limits(**kw)), kw
    for r in ((1, 0), (0, 1)):
        lim = make_trunk_limits()
        lim.reserved[0], lim.reserved[1] = r
        assert ref.limits_refused(lim)
    assert ref.limits_refused(None, body=(0.0, 0.175)) and ref.limits_refused(None, body=(0.4, 2.5)) and ref.limits_refused(None, body=(np.nan, 0.1))
    assert not ref.limits_refused(make_trunk_limits(half_length=0.3), body=(0.0, 0.175))
    # a query's half extent, else the limits', else half the params' — each axis on its own
    lim = make_trunk_limits(half_length=0.3)
    assert ref.default_half_extents(None) == (0.5 * np.float64(np.float32(0.4387)), 0.5 * np.float64(np.float32(0.175)))
    assert ref.default_half_extents(lim) == (np.float64(np.float32(0.3)), 0.5 * np.float64(np.float32(0.175)))
    feet = stance(grid(), 4, 8, 5, 9)
    assert ref.frame(feet, 0.0, 0.125, lim)[2:4] == (np.float64(np.float32(0.3)), 0.125)
    assert ref.frame(feet, 0.75, -1.0, lim)[2:4] == (0.75, 0.5 * np.float64(np.float32(0.175)))


def test_documented_sizes_and_constants():
    assert (_capi.TRUNK_QUERY_DTYPE.itemsize, C.sizeof(_capi.TrunkLimits), _capi.TRUNK_RECORD_DTYPE.itemsize,
            _capi.TRUNK_SUMMARY_DTYPE.itemsize, C.sizeof(_capi.TrunkOut)) == (112, 48, 56, 40, 16)
    assert _capi.ABI_VERSION == 5 and _capi.lib().fpe_abi_version() == 5
    assert (_capi.TRUNK_STANCE, _capi.TRUNK_OFF_MAP, _capi.TRUNK_EMPTY, _capi.TRUNK_UNKNOWN, _capi.TRUNK_UNDER_CLEARANCE,
            _capi.TRUNK_OVER_SLOPE, _capi.TRUNK_DEGENERATE, _capi.TRUNK_REFUSED) == (
        ref.STANCE, ref.OFF_MAP, ref.EMPTY, ref.UNKNOWN, ref.UNDER_CLEARANCE, ref.OVER_SLOPE, ref.DEGENERATE, ref.REFUSED) == (
        1, 2, 4, 8, 16, 32, 64, 128)
    assert (_capi.TRUNK_MAX_HALF_EXTENT, _capi.TRUNK_MAX_CELLS, _capi.TRUNK_MAX_SLOPE) == (ref.MAX_HALF_EXTENT, ref.MAX_CELLS, ref.MAX_SLOPE)
    assert ref.BODY == (_capi.params_yaml()["length"][0], _capi.params_yaml()["width"][0])
    q = make_trunk_queries([[[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]], 0.3, 0.1)
    assert q.dtype == _capi.TRUNK_QUERY_DTYPE and q["feet"][0, 2].tolist() == [7, 8, 9]
    assert (q["half_length"][0], q["half_width"][0], q["reserved"][0].tolist()) == (np.float32(0.3), np.float32(0.1), [0, 0])


def test_limits_defaults():
    tl = _capi.TrunkLimits(1.0, 2.0, 3.0, 4.0, 5.0, 6.0, (C.c_int32 * 2)(7, 8))
    assert _capi.lib().fpe_trunk_limits_defaults(C.byref(tl)) == _capi.FPE_OK
    assert (tl.min_clearance, tl.max_slope_x, tl.max_slope_y, tl.ride_height, tl.half_length, tl.half_width, list(tl.reserved)) == (
        -INF, INF, INF, 0.0, 0.0, 0.0, [0, 0])
    assert _capi.lib().fpe_trunk_limits_defaults(None) == _capi.FPE_E_INVALID_ARG
    assert bytes(make_trunk_limits()) == bytes(tl) and ref.limits_tuple(None) == ref.limits_tuple(tl)
    assert bytes(_capi.trunk_limits_defaults()) == bytes(tl) and _capi.trunk_limits_defaults(ride_height=0.3).ride_height == 0.3


def test_plan_bound_stances_on_all_eight_cycle_ok_patterns():
    """n = 3: record (b, g) is a stance iff cycle g committed; its feet are that cycle's four nominal records."""
    patterns = list(itertools.product((0, 1), repeat=3))
    B, n = len(patterns), 3
    rng = np.random.default_rng(3)
    nominal = np.zeros((B, n, 4), _capi.FOOTHOLD_DTYPE)
    nominal["x"], nominal["y"] = rng.uniform(-1, 1, (B, n, 4)), rng.uniform(-1, 1, (B, n, 4))
    nominal["z"] = rng.uniform(-0.2, 0.2, (B, n, 4)).astype(np.float32)
    ok = np.array(patterns, np.uint8)
    q, is_stance = ref.stances_from_products(nominal, ok)
    assert np.array_equal(is_stance, ok.astype(bool))
    for b, pat in enumerate(patterns):
        for g in range(n):
            if not pat[g]:
                assert q[b, g].tobytes() == bytes(112)
                continue
            for leg in range(4):
                assert q["feet"][b, g, leg].tolist() == [nominal["x"][b, g, leg], nominal["y"][b, g, leg], np.float64(nominal["z"][b, g, leg])]
            assert q["half_length"][b, g] == 0 and q["half_width"][b, g] == 0 and not q["reserved"][b, g].any()
    # records and summary on a flat map: zero records keep their cycle id, and the summary runs over the stances alone
    g = ref.Grid(np.zeros((120, 120), np.float32), 0.02)
    lim = make_trunk_limits(max_slope_x=0.5)
    rec = ref.plan_records(g, nominal, ok, lim)
    assert np.array_equal(rec["gait_cycle_id"], np.broadcast_to(np.arange(n, dtype=np.uint8), (B, n)))
    assert np.array_equal((rec["flags"] & ref.STANCE) != 0, is_stance) and not rec["flags"][~is_stance].any()
    for idx in zip(*np.nonzero(is_stance)):
        want = ref.stance_record(g, q["feet"][idx], 0.0, 0.0, lim)
        want["gait_cycle_id"] = idx[1]
        assert rec[idx].tobytes() == want.tobytes()
    s = ref.summary_from_records(rec)
    assert s["n_stances"].tolist() == [sum(p) for p in patterns]
    assert s[0].tobytes() == np.float64(INF).tobytes() + bytes(28) + b"\xff" + bytes(3)
    for b in range(1, B):
        st = rec[b][is_stance[b]]
        bad = (st["flags"] & (ref.OVER_SLOPE | ref.UNDER_CLEARANCE)) != 0
        assert s["min_clearance"][b] == st["clearance"].min() and s["max_abs_slope_x"][b] == np.abs(st["slope_x"]).max()
        assert s["max_abs_slope_y"][b] == np.abs(st["slope_y"]).max() and s["n_bad"][b] == bad.sum()
        assert s["first_bad_cycle"][b] == (st["gait_cycle_id"][bad].min() if bad.any() else 255)
    assert 0 < s["n_bad"].sum() < s["n_stances"].sum()
