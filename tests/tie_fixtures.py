"""Exact-tie inputs for the chained plan: every comparison of a distance with a radius, and of a cell centre with a
rectangle edge, is decided on an exact tie somewhere in these fixtures.

Resolutions are 2^-5, 2^-6 and 2^-7 m, the map position is a multiple of the resolution, and every length of
fpe_params is a small multiple of the resolution that f32 holds exactly, so feet, cell centres, cell edges and radii are
dyadic numbers and nothing is rounded anywhere: a cell centre lies ON the search circle, a rectangle edge ON a cell edge.
One third of the poses sit on cell centres, one third on cell corners, one third half a cell off in x only.

The foot radius decides the kernel family.  A foot radius of exactly res or 2 res puts lattice points on the foot
disc's circle, so the host cannot prove the offset table (derive_foot_offsets) and the plan takes a direct kernel with the
literal disc walk; the bit-window families need a disc without a lattice point on its circle and get 1/2, 15/16 and 3/2
of the resolution (15/16 is inside the 3x3-only variant's [0.9, 1] band).

tests/test_cpu_tie_fixtures.py proves on the oracle alone that the ties decide outcomes (a radius one f32 ulp shorter
changes at least 1 % of the legs); tests/test_gpu_plan_matrix.py runs the engine on the same fixtures."""
import numpy as np

from quadrupedal_foothold_planner_amd import _capi, synth

# name, log2(1 / res), rows, cols, map position in cells, k = searchRadius / res, footRadius / res, per-leg radii and
# polygons mixed, the kernel describe_plan() must name (with the side of its bit window: k + 1 rows each way — the tie row
# of bits_window_halfwidth's `reach` — or k + footReach where that is more), seed
_TABLE = [
    ("r5_k4_half", 5, 160, 192, (0, 0), 4, 0.5, False, "plan_bits_kernel<2, false> (8 lanes per leg, 11 x 11 bit window", 101),
    ("r5_k6_mid", 5, 160, 192, (96, -64), 6, 0.9375, False, "plan_bits_kernel<2, true> (8 lanes per leg, 15 x 15 bit window", 102),
    ("r5_k4_rf1", 5, 160, 192, (0, 0), 4, 1.0, True, "plan_chained_kernel<8, false> (direct)", 103),
    ("r6_k8_rf15", 6, 320, 288, (0, 0), 8, 1.5, False, "plan_bits_kernel<3, false> (8 lanes per leg, 19 x 19 bit window", 104),
    ("r6_k10_mid", 6, 320, 288, (-128, 192), 10, 0.9375, False, "plan_bits_kernel<3, true> (8 lanes per leg, 23 x 23 bit window", 105),
    ("r6_k14_half", 6, 320, 288, (0, 0), 14, 0.5, True, "plan_bits_kernel<4, false> (8 lanes per leg, 31 x 31 bit window", 106),
    ("r6_k8_rf2", 6, 320, 288, (64, 64), 8, 2.0, True, "plan_chained_kernel<8, false> (direct)", 107),
    ("r7_k20_rf15", 7, 512, 448, (0, 0), 20, 1.5, True, "plan_bits_seq_kernel<1, 2> (one wavefront per pose, 43 x 43 bit window", 108),
    ("r7_k36_half", 7, 512, 448, (256, -384), 36, 0.5, True, "plan_bits_seq_kernel<2, 3> (one wavefront per pose, 75 x 75 bit window", 109),
    ("r7_k20_rf2", 7, 512, 448, (0, 0), 20, 2.0, False, "plan_sequential_kernel (direct", 110),
]
NAMES = [t[0] for t in _TABLE]
N_CYCLES = 5
N_POSES = 60


def make(name):
    """One fixture: dict(res, pos, params, trav, elev, poses, n, maxleg, kernel, k)."""
    _, e, rows, cols, pos_cells, k, rf_cells, mixed, kernel, seed = _TABLE[NAMES.index(name)]
    res = 2.0 ** -e
    rng = np.random.default_rng(seed)
    pos = (pos_cells[0] * res, pos_cells[1] * res)
    u = 2.0 ** -5  # every body length is a multiple of the coarsest resolution, hence of all three
    p = _capi.params_yaml()
    p["searchRadius"] = np.float32(k * res)
    p["footRadius"] = np.float32(rf_cells * res)
    p["length"], p["width"], p["l1"] = np.float32(14 * u), np.float32(8 * u), np.float32(2 * u)
    p["stepLength"], p["skew"] = np.float32(6 * u), np.float32(1 * u)
    p["h"] = float(rng.choice([0.0, 2.0 ** -6]))
    p["lateralDrift"] = float(rng.choice([0.0, 2.0 ** -7, -(2.0 ** -7)]))
    p["RF_FIRST"] = int(rng.integers(0, 2))
    # fewer bad cells under a larger foot disc, so that roughly half of the discs stay clear and searches both succeed and fail
    bad_frac = {0.5: 0.3, 0.9375: 0.3, 1.0: 0.12, 1.5: 0.08, 2.0: 0.05}[rf_cells]
    trav, elev = synth.rough_map(rows, cols, res, seed=seed, position=pos, nan_frac=0.01, bad_frac=bad_frac, stair_period=1.1)
    # poses in cells relative to the map position; rows and cols are even, so integers are cell corners and integers + 1/2 are
    # cell centres.  The range overhangs the map by a few cells on every side: clipped windows and centres outside.
    B = N_POSES
    ix = rng.integers(-rows // 2 - 6, rows // 2 - 30, B).astype(np.float64)
    iy = rng.integers(-cols // 2 - 6, cols // 2 + 6, B).astype(np.float64)
    third = np.arange(B) % 3
    ix[third == 0] += 0.5
    iy[third == 0] += 0.5  # cell centres
    ix[third == 2] += 0.5  # half a cell off in x only; third == 1 stays on the corners
    poses = np.zeros(B, dtype=_capi.POSE_DTYPE)
    poses["position"][:, 0] = pos[0] + ix * res
    poses["position"][:, 1] = pos[1] + iy * res
    poses["position"][:, 2] = rng.integers(-8, 9, B) * 2.0 ** -6
    poses["gait"] = rng.integers(0, 2, B)
    maxleg = 0.0
    if mixed:  # per-leg radii that are exact multiples of the resolution too (0 keeps searchRadius), both polygon kinds
        poses["leg_polygon_kind"] = rng.integers(0, 2, (B, 4))
        kk = rng.integers(max(2, k // 2), k + 1, (B, 4))
        kk[rng.random((B, 4)) < 0.4] = 0
        poses["leg_search_radius"] = (kk * res).astype(np.float32)
        maxleg = k * res
    return dict(name=name, res=res, pos=pos, params=p, trav=trav, elev=elev, poses=poses, n=N_CYCLES, maxleg=maxleg, kernel=kernel,
                k=k)


def one_ulp_shorter(fx):
    """The same fixture with every search radius one f32 ulp below its tie value: (params, poses)."""
    p = fx["params"].copy()
    p["searchRadius"] = np.nextafter(np.float32(p["searchRadius"][0]), np.float32(0))
    poses = fx["poses"].copy()
    r = poses["leg_search_radius"]
    poses["leg_search_radius"] = np.where(r > 0, np.nextafter(r, np.float32(0)), r)
    return p, poses
