"""Map positions far from the origin, shared by tests/test_host_switches.py, tests/test_cpu_far_origin.py and
tests/test_gpu_far_origin.py, and the magnitudes at which the host's derivations (csrc/fpe_host.cpp) change their mind —
restated here from the formulas in that file's comments, not read off its results.

A robot-centric map that grid_map::move carries along has its position grow with the distance walked: 1e3 .. 1e6 m in an
odom or UTM frame.  Every coordinate stays below the 1e6 guard (centre_usable) unless a test is about the guard."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)

NEAR = (1234.56, -987.25)
FAR = (-999000.37, 998000.11)
FAR_DYADIC = (31000000 * 2.0 ** -5, -30000000 * 2.0 ** -5)  # (968750, -937500): every cell centre of a 2^-5 m map is exact


def foot_gap(rf32, res):
    """Smallest |d^2 - rf^2| over the lattice offsets d^2 = (a^2 + b^2) res^2 (derive_foot_offsets)."""
    rf = float(np.float32(rf32))
    reach = int(np.ceil(rf / res)) + 1
    a = np.arange(-reach, reach + 1, dtype=np.float64)
    d2 = (a[:, None] * a[:, None] + a[None, :] * a[None, :]) * (res * res)
    return float(np.abs(d2 - rf * rf).min())


def foot_robust_flip_maxabs(rf32, res):
    """derive_foot_offsets: tol = 4 (rf + 2 res) * (4 maxAbs eps) + 1e-9 rf^2 + 8 eps rf^2; the offset table is refused
    (footRobust = 0) once tol >= the gap of the lattice offset nearest the circle.  -> the maxAbs at which tol = gap."""
    rf = float(np.float32(rf32))
    rf2 = rf * rf
    return (foot_gap(rf32, res) - 1e-9 * rf2 - 8.0 * EPS * rf2) / (16.0 * (rf + 2.0 * res) * EPS)


def foot_robust_flip_posx(rf32, res, rows, cols):
    """The map position (x, with y = 0) of a rows x cols map at which footRobust flips:
    maxAbs = max(|posX| + lenX, |posY| + lenY) + rf + res."""
    rf = float(np.float32(rf32))
    px = foot_robust_flip_maxabs(rf32, res) - rows * res - rf - res
    assert px + rows * res > cols * res
    return px


def reach_tie_flip_mag(R32, res):
    """bits_window_halfwidth: reach(R) = ceil(q), q = R / res, and round(q) + 1 once |q - round(q)| <= slack =
    64 eps mag / res + 1e-12.  A quotient just BELOW an integer gains a row there; one just above already has it from the
    ceil.  -> (mag at which slack = |q - round(q)|, q)."""
    q = float(np.float32(R32)) / res
    return (abs(q - round(q)) - 1e-12) * res / (64.0 * EPS), q


def mag_of(px, py, rows, cols, res, R32, rf32):
    return abs(px) + rows * res + abs(py) + cols * res + float(np.float32(R32)) + float(np.float32(rf32)) + 1.0


def yaml_foot_positions(rows=200, cols=180, res=0.02, rf32=0.02):
    """BELOW and ABOVE: 0.5 and 1.25 times the x at which the yaml foot (f32(0.02) on 2 cm cells: the offset (1, 0) lies
    1.8e-11 m^2 off the circle) loses its proved offset table on a rows x cols map — about 41 km and 103 km.  (The same
    foot on 1 cm and 0.5 cm cells has the offsets (2, 0) and (4, 0) as close and a tolerance that grows more slowly with
    rf + 2 res: those tables go at 123 km and 164 km, between ABOVE and FAR.)"""
    px = foot_robust_flip_posx(rf32, res, rows, cols)
    return (round(0.5 * px, 2), -987.25), (round(1.25 * px, 2), -987.25)


BELOW, ABOVE = yaml_foot_positions()
POSITIONS = {"near": NEAR, "below": BELOW, "above": ABOVE, "far": FAR}


def moved(poses, pos):
    """A copy of engine poses translated with the map."""
    out = poses.copy()
    out["position"][:, 0] += pos[0]
    out["position"][:, 1] += pos[1]
    return out


def kernel_table(path=None):
    """profiles/far_origin_kernels.txt: {(matrix row, position name): the kernel name describe_plan() begins with}."""
    import os

    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "far_origin_kernels.txt")
    table = {}
    with open(path) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                row, pos, kernel = line.rstrip("\n").split(None, 2)
                table[(row, pos)] = kernel
    return table


def tie_kernel_far(fx):
    """The kernel a fixture of tests/tie_fixtures.py names with its map moved by FAR_DYADIC: its own, except at 2^-7 m, where
    the index quotients (|x| + |y| + 2e6) / res no longer leave bits_window_halfwidth's condition (4) its room."""
    return "plan_sequential_kernel (direct" if fx["res"] == 2.0 ** -7 else fx["kernel"]


def predicted_kernel(row, consts):
    """What select_plan_kernel (csrc/fpe_plan_launch.hpp) names for a plain plan from the host's switches: the row's own
    bit-window kernel while the window is proved at the row's half-width; without a window a direct kernel — eight lanes
    per leg while the LDS tile has at most 32 x 32 cells, one wavefront per pose beyond — whose 3x3-only variant needs
    the proved one-cell table."""
    if consts["winH"] > 0:
        assert consts["winH"] == row.winH, (row.id, consts)
        return row.kernel.split(" (")[0]
    if consts["tileW"] * consts["tileW"] > 1024:
        return "plan_sequential_kernel"
    mid = consts["midCellInside"] and float(np.float32(row.rf)) <= row.res and consts["footRobust"]
    return "plan_chained_kernel<8, %s>" % ("true" if mid else "false")


# ---- the cases of tests/test_gpu_far_origin.py that have a Python reference (conditions: tests/test_cpu_far_origin.py) ------------
def _cached(fn):
    import functools

    return functools.lru_cache(maxsize=None)(fn)


@_cached
def stride_case(row_id, pos=FAR):
    """tests/stride_reference.py's case of a matrix row with the map at `pos` and the poses moved with it."""
    from tests import resume_reference as rref
    from tests import util

    c = dict(rref.case(row_id))
    c["pos"] = pos
    c["poses"] = moved(c["poses"], pos)
    c["oposes"] = util.to_oracle_poses(c["poses"])
    return c


def omap_of(c, second_map=False):
    from oracle import fpo

    return fpo.OracleMap(c["trav2" if second_map else "trav"], c["elev2" if second_map else "elev"], c["row"].res, c["pos"])


BEAM_NAMES = ("w7_gen", "w16_seq")


@_cached
def beam_case(name, pos=FAR):
    """tests/beam_reference.py's case (roots from the poses) with the map at `pos`."""
    from tests import beam_reference as bref
    from tests import util

    c = dict(bref.case(name))
    assert c["states"] is None
    c["pos"] = pos
    c["roots"] = moved(c["roots"], pos)
    c["oroots"] = util.to_oracle_poses(c["roots"])
    return c


@_cached
def beam_reference(name, pos=FAR):
    from tests import beam_reference as bref

    c = beam_case(name, pos)
    return bref.beam(omap_of(c), c["oparams"], c["oroots"], c["options"], c["S"], c["k"], c["W"], c["weights"], None)


@_cached
def rank_case(pos=FAR):
    """tests/rank_reference.py's main case with the map at `pos`: inputs, the oracle's plan and the reference summaries."""
    from oracle import fpo
    from quadrupedal_foothold_planner_amd import _capi
    from tests import rank_reference as ref
    from tests import util

    trav, elev, res, poses, n = ref.main_inputs()
    poses = moved(poses[:48], pos)
    params = _capi.params_yaml()
    params["footRadius"] = np.float32(0.008)  # a one-cell foot whose table stays proved out there: the bit-window ranking kernel
    omap = fpo.OracleMap(trav, elev, res, pos)
    op, opo = util.to_oracle_params(params), util.to_oracle_poses(poses)
    plan = omap.plan(op, opo, n, threads=4)
    plan["pose_status"] = omap.pose_status(op, opo)
    return dict(trav=trav, elev=elev, res=res, pos=pos, poses=poses, n=n, params=params, plan=plan,
                summary=ref.summary_from_oracle(omap, op, opo, n, plan=plan))
