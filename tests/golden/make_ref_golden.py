#!/usr/bin/env python3
"""Generate tests/golden/ref/*.npz: small inputs and what the REFERENCE's own planner computes on them.

PROVENANCE: oracle/_ref/ref_driver is the reference's FootholdPlanner.cpp compiled verbatim, from where it lies, against
the shim headers of oracle/ref_shim/ (recipe: oracle/Makefile).  Each fixture stores its inputs (the map itself, the
parameters, the start poses or queries) and the reference's outputs — nothing here is computed by the oracle.  Whether a
centroid query ended whole-region-valid (0), in one of the four cases (1-4), with no case (5) or without a submap (6) is
read off the reference's outputs alone (refcase.reference_centroid_class); the oracle is consulted for ONE thing, after
its outputs have been found equal to the reference's: WHICH of the cases 1-4 ran, which the reference reports through
stdout only.

PINNED by these vectors: the logic of FootholdPlanner.cpp (checkFoothold, checkFootholdUseCentroidMethod,
getFootholdMeanHeight, getDefaultFootholdNext, setFirstGait, getGaitCycleSearchGridMap, getMapIndex, the per-cycle driver
of globalFootholdPlan for all three tracks, the commit rule, the service's return value, and the opt track's objective
and eight constraints — the reference's own nloptFunc / nloptConstraint1..8 are what the shim optimiser calls).
STILL UNPINNED: grid_map_core's semantics (the shim forwards to oracle/fpo_gridmap.hpp), NLopt's COBYLA (the shim's
optimiser is the build-defined lattice rule), the traversability filter package, everything build-defined.

All cases: trot gait, rectangle polygons, no per-leg radii (the reference has nothing else); h_ = 0.01 and the lateral
drift -0.007 are constants of the reference.  Needs the reference tree ($REF, default /root/reference).
Run from the repository root:  python tests/golden/make_ref_golden.py [OUTDIR]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import fpo  # noqa: E402
from tests import refcase  # noqa: E402
from tests.conftest import yaml_params  # noqa: E402
from tests.golden import make_golden  # noqa: E402

GOLDEN = os.path.dirname(os.path.abspath(__file__))
MAX_ROWS, MAX_COLS = 160, 128
MAX_BYTES = 64 * 1024


def opt_variant(name):
    op = fpo.opt_params_yaml()
    for k, v in make_golden.OPT_VARIANTS[name].items():
        op[k] = v
    return op


def quantised_map(rows, cols, res, seed, position=(0.0, 0.0), bad=0.06, stairs=True):
    """A hostile little map whose elevation takes few distinct values (it compresses): steps across x, holes, bad
    cells, NaN and +-inf traversability, NaN and >= 10 elevations."""
    assert rows <= MAX_ROWS and cols <= MAX_COLS
    rng = np.random.default_rng(seed)
    trav = np.ones((rows, cols), np.float32)
    elev = (np.round(rng.standard_normal((rows, cols)) * 4) / 128.0).astype(np.float32)
    if stairs:
        for k in range(1, 5):
            r0 = rows * k // 5
            trav[r0:r0 + 2, :] = 0.2
            elev[:r0, :] += np.float32(0.125)
    trav[rows // 2:rows // 2 + max(3, rows // 20), cols // 4:cols // 4 + max(4, cols // 10)] = 0.05
    badmask = rng.random((rows, cols)) < bad
    trav[badmask] = (np.round(rng.uniform(0, 0.6, size=int(badmask.sum())) * 64) / 64).astype(np.float32)
    trav[rng.random((rows, cols)) < 0.02] = np.nan
    trav[rng.random((rows, cols)) < 0.004] = -np.inf
    trav[rng.random((rows, cols)) < 0.004] = np.inf
    elev[rng.random((rows, cols)) < 0.02] = np.nan
    elev[rng.random((rows, cols)) < 0.01] = 11.0
    elev[rng.random((rows, cols)) < 0.003] = 10.0
    return trav, elev


def scaled_params(scale, **over):
    """yaml parameters with the robot geometry scaled (as trot_1cm_r015 does) so that a stance fits a small map."""
    p = yaml_params()
    for k in ("searchRadius", "stepLength", "length", "width", "l1", "skew", "footRadius"):
        p[k] = np.float32(float(p[k][0]) * scale)
    for k, v in over.items():
        p[k] = v if k == "RF_FIRST" else np.float32(v)
    return p


def code_default_params():
    return make_golden.params_for("code")


def edge_poses(rows, cols, res, position, params, rng, n):
    """Start poses all over the map and past it: windows clipped by the border, the gait-cycle submap failing in cycle 0
    (centre outside the map) and in a later cycle (walking out of the +x edge), and poses on the -y edge that the lateral
    drift of -0.007 per cycle carries out."""
    lx, ly = rows * res, cols * res
    step = float(params["stepLength"][0])
    xs = rng.uniform(position[0] - 0.5 * lx - 0.5 * step, position[0] + 0.5 * lx + 0.3 * step, n)
    ys = rng.uniform(position[1] - 0.5 * ly - 0.02, position[1] + 0.5 * ly + 0.02, n)
    k = n // 4
    xs[:k] = position[0] + 0.5 * lx - rng.uniform(1.5, 4.5, k) * step   # leaves the +x edge after a few cycles
    ys[k:2 * k] = position[1] - 0.5 * ly + rng.uniform(0.001, 0.03, k)  # on the -y edge: the drift carries it out
    xs[k:2 * k] = position[0] + rng.uniform(-0.45, -0.1, k) * lx
    return np.stack([xs, ys, np.round(rng.uniform(-0.2, 0.2, n) * 64) / 64], axis=1)


def tie_case(name, e, rows, cols, pos_cells, k, rf_cells, rf_first, seed):
    """The exact-tie geometry of tests/tie_fixtures.py for the trot gait: resolution 2^-e, dyadic lengths, poses on cell
    centres, cell corners and half a cell off in x.  (The reference's drift, -0.007, is not dyadic: the y ties hold in
    the first cycle only, the x ties in every cycle.)  Fewer bad cells than tie_fixtures.py sprinkles: with 30 % of them
    a third of the start poses commit coincident feet, where the reference is undefined (screen_poses)."""
    from quadrupedal_foothold_planner_amd import synth

    res = 2.0 ** -e
    rng = np.random.default_rng(seed)
    pos = (pos_cells[0] * res, pos_cells[1] * res)
    u = 2.0 ** -5
    p = yaml_params()
    p["searchRadius"], p["footRadius"] = np.float32(k * res), np.float32(rf_cells * res)
    p["length"], p["width"], p["l1"] = np.float32(14 * u), np.float32(8 * u), np.float32(2 * u)
    p["stepLength"], p["skew"] = np.float32(6 * u), np.float32(1 * u)
    p["RF_FIRST"] = rf_first
    trav, elev = synth.rough_map(rows, cols, res, seed=seed, position=pos, nan_frac=0.01,
                                 bad_frac={0.5: 0.12, 0.9375: 0.12, 1.0: 0.08}[rf_cells], stair_period=1.1)
    elev = (np.round(elev.astype(np.float64) * 256) / 256).astype(np.float32)
    B = 18
    ix = rng.integers(-rows // 2 - 4, rows // 2 - 24, B).astype(np.float64)
    iy = rng.integers(-cols // 2 - 3, cols // 2 + 3, B).astype(np.float64)
    third = np.arange(B) % 3
    ix[third == 0] += 0.5
    iy[third == 0] += 0.5
    ix[third == 2] += 0.5
    poses = np.stack([pos[0] + ix * res, pos[1] + iy * res, rng.integers(-8, 9, B) * 2.0 ** -6], axis=1)
    return dict(name=name, mode="service", trav=trav, elev=elev, res=res, position=pos, params=p, poses=poses, n=3,
                variants=["yaml"])


def leg_queries(rows, cols, res, position, params, rng, n_check, n_centroid, n_height):
    """Open-loop queries: checkFoothold with its own search radius and rectangle (some rectangles displaced from the
    centre, as the nominal track's are), the centroid method, mean heights — centres inside, on and past the border."""
    lx, ly = rows * res, cols * res
    n = n_check + n_centroid + n_height
    q = np.zeros(n, refcase.QUERY_DTYPE)
    q["kind"][n_check:n_check + n_centroid] = 1
    q["kind"][n_check + n_centroid:] = 2
    q["cx"] = rng.uniform(position[0] - 0.5 * lx - 2 * res, position[0] + 0.5 * lx + 2 * res, n)
    q["cy"] = rng.uniform(position[1] - 0.5 * ly - 2 * res, position[1] + 0.5 * ly + 2 * res, n)
    lattice = rng.random(n) < 0.25  # lattice-aligned centres: exact ties in the index arithmetic
    q["cx"][lattice] = np.round(q["cx"][lattice] / res) * res
    q["cy"][lattice] = np.round(q["cy"][lattice] / res) * res
    R = float(params["searchRadius"][0])
    q["foot_radius"] = params["footRadius"][0]
    q["foot_radius"][n_check + n_centroid:] = rng.choice([0.4, 1.0, 1.5, 3.6], n_height).astype(np.float32) * np.float32(res)
    q["search_radius"] = rng.uniform(0.4 * R, R, n).astype(np.float32)
    q["search_radius"][rng.random(n) < 0.3] = np.float32(R)
    for k in range(n):
        r = q["search_radius"][k]  # float32, promoted per use as cpp:2501-2508 does
        dx, dy = (rng.uniform(-0.5, 0.5) * float(r), rng.uniform(-0.3, 0.3) * float(r)) if rng.random() < 0.5 else (0.0, 0.0)
        cx, cy = q["cx"][k] + dx, q["cy"][k] + dy
        q["vx"][k] = (cx + r, cx + r, cx - r, cx - r)
        q["vy"][k] = (cy + 0.5 * r, cy - 0.5 * r, cy - 0.5 * r, cy + 0.5 * r)
    return q


def cases():
    out = []
    # ---- the four committed trot goldens, with the opt variants of make_golden.py: cross-checks the oracle goldens ----
    for name in ("trot_2cm", "trot_1cm_r015", "harsh_2cm", "code_defaults_3cm"):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        # one fixture per variant: each carries the map itself and stays under the size limit
        for v in ["yaml"] if name == "trot_1cm_r015" else ["yaml", "code", "weights"]:
            out.append(dict(name=f"svc_{name}_{v}", mode="service", trav=z["trav"], elev=z["elev"], res=float(z["res"]), position=(0.0, 0.0),
                            params=z["params"].view(fpo.PARAMS_DTYPE), poses=z["poses"].view(fpo.POSE_DTYPE)["pose"], n=int(z["n_cycles"]),
                            variants=[v], base=name))
    # ---- new ones ----
    rng = np.random.default_rng(20261018)
    # 2 cm, yaml defaults, both RF_FIRST, foot disc of ONE cell (radius 0.4 cells), poses over every border
    for rf in (0, 1):
        p = scaled_params(0.5, footRadius=0.4 * 0.02, RF_FIRST=rf)
        trav, elev = quantised_map(128, 96, 0.02, 301 + rf)
        out.append(dict(name=f"svc_edges_2cm_rf{rf}", mode="service", trav=trav, elev=elev, res=0.02, position=(0.0, 0.0), params=p,
                        poses=edge_poses(128, 96, 0.02, (0.0, 0.0), p, rng, 24), n=6, variants=["yaml", "code"][rf:rf + 1]))
    # 1 cm, off-origin map, foot disc of 9 cells (radius 1.5 cells)
    pos = (3.37, -1.254)
    p = scaled_params(0.4, footRadius=1.5 * 0.01)
    trav, elev = quantised_map(160, 128, 0.01, 303, pos)
    out.append(dict(name="svc_offorigin_1cm", mode="service", trav=trav, elev=elev, res=0.01, position=pos, params=p,
                    poses=edge_poses(160, 128, 0.01, pos, p, rng, 20), n=5, variants=["yaml"]))
    # 5 mm, foot disc of 45 cells (radius 3.7 cells), RF_FIRST
    p = scaled_params(0.15, footRadius=3.7 * 0.005, RF_FIRST=1)
    trav, elev = quantised_map(160, 128, 0.005, 304, (-0.4, 0.2), bad=0.02)
    out.append(dict(name="svc_fine_5mm", mode="service", trav=trav, elev=elev, res=0.005, position=(-0.4, 0.2), params=p,
                    poses=edge_poses(160, 128, 0.005, (-0.4, 0.2), p, rng, 16), n=4, variants=["code"]))
    # 3 cm, the code's own defaults (readParameters' fallbacks)
    p = code_default_params()
    trav, elev = quantised_map(120, 100, 0.03, 305)
    out.append(dict(name="svc_code_3cm", mode="service", trav=trav, elev=elev, res=0.03, position=(0.0, 0.0), params=p,
                    poses=edge_poses(120, 100, 0.03, (0.0, 0.0), p, rng, 20), n=5, variants=["code", "yaml"]))
    # the non-dyadic 2.37 cm
    p = scaled_params(0.6, RF_FIRST=1)
    trav, elev = quantised_map(150, 110, 0.0237, 306, (0.731, 0.0119))
    out.append(dict(name="svc_nondyadic_237", mode="service", trav=trav, elev=elev, res=0.0237, position=(0.731, 0.0119), params=p,
                    poses=edge_poses(150, 110, 0.0237, (0.731, 0.0119), p, rng, 20), n=5, variants=["weights"]))
    # exact ties
    out.append(tie_case("svc_tie_r5_k4_half", 5, 160, 128, (0, 0), 4, 0.5, 0, 401))
    out.append(tie_case("svc_tie_r5_k6_mid", 5, 160, 128, (96, -64), 6, 0.9375, 1, 402))
    out.append(tie_case("svc_tie_r5_k4_rf1", 5, 160, 128, (0, 0), 4, 1.0, 0, 403))
    # ---- legs ----
    for name, rows, cols, res, pos, scale, seed in (("legs_2cm", 96, 64, 0.02, (0.0, 0.0), 1.0, 501),
                                                    ("legs_1cm_offorigin", 128, 96, 0.01, (3.37, -1.254), 0.5, 502),
                                                    ("legs_nondyadic_237", 90, 70, 0.0237, (0.731, 0.0119), 1.0, 503),
                                                    ("legs_5mm_bigfoot", 128, 96, 0.005, (0.0, 0.0), 0.25, 504)):
        p = scaled_params(scale, footRadius=3.7 * res) if name == "legs_5mm_bigfoot" else scaled_params(scale)
        trav, elev = quantised_map(rows, cols, res, seed, pos, bad=0.12 if name != "legs_5mm_bigfoot" else 0.01)
        out.append(dict(name=name, mode="legs", trav=trav, elev=elev, res=res, position=pos, params=p,
                        queries=leg_queries(rows, cols, res, pos, p, np.random.default_rng(seed), 240, 200, 60)))
    return out + far_cases()


FAR_POSITIONS = ((1234.56, -987.25), (123456.789, -98765.4321), (-999000.37, 998000.11))


def far_cases():
    """Maps far from the origin — where a robot-centric map in an odom or UTM frame lies.  Every case draws from a
    generator of its own (the shared one of cases() is consumed as before).  Every coordinate a chain can reach stays
    below 1e6: the guard there (centreUsable) is the oracle's definition, not the reference's."""
    near, mid, far = FAR_POSITIONS
    out = []

    def svc(name, rows, cols, res, pos, scale, n, B, variant, seed, map_seed, **over):
        p = scaled_params(scale, **over)
        trav, elev = quantised_map(rows, cols, res, map_seed, pos)
        out.append(dict(name=name, mode="service", trav=trav, elev=elev, res=res, position=pos, params=p,
                        poses=edge_poses(rows, cols, res, pos, p, np.random.default_rng(seed), B), n=n, variants=[variant]))

    # 2 cm at 1.2 km.  Pose 8 derails its opt track in cycle 4: the optimiser keeps the index of an untouched centroid
    # result, the point (0, 0), which this map does not contain, and the mean height is asked for at (0, 0)
    # (oracle/fpo_planner.cpp, getFootholdMeanHeight)
    svc("svc_far_2cm_1km", 128, 96, 0.02, near, 0.5, 5, 12, "yaml", 7, 900)
    svc("svc_far_1cm_123km", 160, 128, 0.01, mid, 0.4, 4, 10, "yaml", 8, 900, footRadius=1.5 * 0.01)  # foot disc of 9 cells
    svc("svc_far_237_999km", 150, 110, 0.0237, far, 0.6, 4, 10, "weights", 9, 900, RF_FIRST=1)
    svc("svc_far_2cm_999km", 128, 96, 0.02, far, 0.5, 5, 12, "code", 10, 902)
    # exact ties at a dyadic position 9.7e5 m out (2^-5 m cells: every cell centre and corner is exact in f64)
    out.append(tie_case("svc_far_tie_r5_k4", 5, 160, 128, (31000000, -30000000), 4, 0.9375, 1, 404))
    for name, rows, cols, res, pos, scale, seed in (("legs_far_2cm_123km", 96, 64, 0.02, mid, 1.0, 505),
                                                    ("legs_far_5mm_999km", 128, 96, 0.005, far, 0.25, 506)):
        p = scaled_params(scale)
        trav, elev = quantised_map(rows, cols, res, seed, pos, bad=0.12)
        out.append(dict(name=name, mode="legs", trav=trav, elev=elev, res=res, position=pos, params=p,
                        queries=leg_queries(rows, cols, res, pos, p, np.random.default_rng(seed), 240, 200, 60)))
    return out


MAX_EXCLUDED_SHARE = 0.05


def screen_poses(c, asan_driver, workdir=None):
    """Input class EXCLUDED from the fixtures, shown by the sanitizer build of the reference (never presumed): start
    poses on which the reference itself has undefined behaviour.  The one report met is

        fpo_gridmap.hpp (getIndexFromPosition): runtime error: -nan is outside the range of representable values of type 'int'

    under getGaitCycleSearchGridMap (cpp:2345) <- globalFootholdPlan (cpp:920): a track has committed coincident feet
    (untouched (0,0,0) results of the centroid method, cpp:1777-1944, or the optimiser's start point kept after NLopt's
    precondition failed), getPolygonCenter divides 0 by 0 (cpp:2457) and the NaN centre reaches grid_map's (int) cast.
    The oracle and the engine DEFINE that case (centreUsable, fpo_planner.cpp); the reference does not, so it cannot
    pin them there.

    NOT excluded, and not reported by the sanitizer build: an opt foot that keeps an untouched centroid result's index on
    a map that does not contain the origin (svc_far_2cm_1km, pose 8, cycle 4).  getFootholdMeanHeight is then asked for
    the height at (0, 0); grid_map's CircleIterator bounds the disc onto the far corner, whose index rounds to `size`, and
    upstream would read one cell past the layer.  The shim returns NaN for that read and counts it (oobReads), so the
    reference built on the shims is defined there: z = 0 + h.  The oracle visits no cell: the same value.
    -> (kept mask over the poses, the reports' first lines)."""
    poses = np.asarray(c["poses"], np.float64).reshape(-1, 3)
    keep = np.ones(poses.shape[0], bool)
    reasons = []
    env_keep = os.environ.get("UBSAN_OPTIONS")
    os.environ["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=0"
    try:
        for v in c["variants"]:
            op = opt_variant(v)
            try:  # the whole case at once; pose by pose only where that aborts
                refcase.run_service(c["trav"], c["elev"], c["res"], c["position"], c["params"], op, poses[keep], c["n"], asan_driver, workdir)
                continue
            except RuntimeError:
                pass
            for b in np.nonzero(keep)[0]:
                try:
                    refcase.run_service(c["trav"], c["elev"], c["res"], c["position"], c["params"], op, poses[b:b + 1], c["n"], asan_driver, workdir)
                except RuntimeError as e:
                    keep[b] = False
                    line = [ln for ln in str(e).splitlines() if "runtime error" in ln or "ERROR: AddressSanitizer" in ln]
                    text = line[0] if line else str(e).splitlines()[0]
                    for mark in ("runtime error", "ERROR: AddressSanitizer"):  # without the file:line:col in front of it
                        if mark in text:
                            text = text[text.index(mark):]
                    reasons.append(text[:160])
    finally:
        if env_keep is None:
            os.environ.pop("UBSAN_OPTIONS", None)
        else:
            os.environ["UBSAN_OPTIONS"] = env_keep
    return keep, reasons


def run_case(c, driver=None, workdir=None, asan_driver=None):
    """-> the fixture's arrays: inputs and the reference's outputs.  With `asan_driver` the start poses are screened
    first (screen_poses); the fixture then holds the kept poses, how many were generated and why the others left."""
    fx = dict(mode=c["mode"], trav=np.asarray(c["trav"], np.float32), elev=np.asarray(c["elev"], np.float32), res=np.float64(c["res"]),
              position=np.asarray(c["position"], np.float64), params=np.asarray(c["params"], fpo.PARAMS_DTYPE).reshape(1))
    if c["mode"] == "legs":
        fx["queries"] = c["queries"]
        fx["result"] = refcase.run_legs(fx["trav"], fx["elev"], c["res"], c["position"], fx["params"], c["queries"], driver, workdir)
        return fx
    fx["poses"] = np.asarray(c["poses"], np.float64).reshape(-1, 3)
    fx["n_generated"] = np.int32(fx["poses"].shape[0])
    if asan_driver is not None:
        keep, reasons = screen_poses(c, asan_driver, workdir)
        fx["poses"] = fx["poses"][keep]
        fx["excluded_reason"] = np.array(sorted(set(reasons)) or [""])
    fx["n_cycles"] = np.int32(c["n"])
    fx["variants"] = np.array(c["variants"])
    if "base" in c:
        fx["base"] = np.array(c["base"])
    for v in c["variants"]:
        op = opt_variant(v)
        fx[v + "/opt_params"] = op
        r = refcase.run_service(fx["trav"], fx["elev"], c["res"], c["position"], fx["params"], op, fx["poses"], c["n"], driver, workdir)
        for k, a in r.items():
            fx[v + "/" + k] = a
    return fx


def coverage(fixtures):
    """The conditions the set must meet, from the reference's outputs alone (the centroid codes are the oracle's labels
    of outputs already found equal)."""
    src = np.zeros(3, np.int64)
    classes = np.zeros(7, np.int64)  # refcase.reference_centroid_class: 0, 1 (= a case 1-4 ran), 5, 6
    accepted = refused = committed = failed = 0
    status = np.zeros(4, np.int64)
    fail_cycles = set()
    for fx in fixtures.values():
        if str(fx["mode"]) == "legs":
            r = fx["result"]
            src += np.bincount(r[r[:, 9] == 0, 1].astype(int), minlength=3)[:3]
            cls = refcase.reference_centroid_class(r)
            classes += np.bincount(cls[cls >= 0], minlength=7)[:7]
            continue
        N = int(fx["n_cycles"])
        for v in fx["variants"]:
            v = str(v)
            ret = fx[v + "/ret"]
            accepted += int(ret.sum())
            refused += int((ret == 0).sum())
            fail_cycles |= set(int(g) for g in fx[v + "/fail_cycle"][ret == 0])
            nc = (fx[v + "/nominal_head"][:, 4] - 4) // 4
            committed += int(nc[ret == 1].sum())
            failed += int((N - nc[ret == 1]).sum())
            for b in range(ret.size):
                n = int(fx[v + "/opt_n"][b])
                status += np.bincount(fx[v + "/opt_rec"][b, :n, 47].astype(int), minlength=4)[:4]
    return dict(sources=src.tolist(), centroid_classes=classes.tolist(), accepted=accepted, refused=refused, committed_cycles=committed, failed_cycles=failed,
                opt_status=status.tolist(), fail_cycles=sorted(fail_cycles))


def assert_coverage(cov, codes=None):
    assert all(n > 0 for n in cov["sources"]), cov
    assert all(cov["centroid_classes"][k] > 0 for k in (0, 1, 5, 6)), cov  # from the reference's outputs alone
    assert cov["accepted"] >= 3 and cov["refused"] >= 3, cov
    assert cov["committed_cycles"] > 0 and cov["failed_cycles"] > 0, cov
    assert all(n > 0 for n in cov["opt_status"][:3]), cov
    assert 0 in cov["fail_cycles"] and any(g > 0 for g in cov["fail_cycles"]), cov
    if codes is not None:
        assert all(n > 0 for n in codes), codes


def centroid_code_counts(fixtures):
    """Oracle labels of the legs fixtures' centroid queries — counted only after the outputs were found equal."""
    codes = np.zeros(7, np.int64)
    for fx in fixtures.values():
        if str(fx["mode"]) != "legs":
            continue
        m = fpo.OracleMap(fx["trav"], fx["elev"], float(fx["res"]), tuple(fx["position"]))
        ora, lab = refcase.oracle_legs(m, fx["params"], fx["queries"])
        refcase.assert_legs_equal(fx["result"], ora, "legs ")
        codes += np.bincount(lab[lab >= 0], minlength=7)[:7]
    return codes.tolist()


def excluded_share(fixtures):
    """(share, excluded, generated) over the generated start poses; the poses of a committed oracle golden count once,
    not once per opt variant."""
    gen = kept = 0
    seen = set()
    for fx in fixtures.values():
        if str(fx["mode"]) != "service":
            continue
        if "base" in fx:
            if str(fx["base"]) in seen:
                continue
            seen.add(str(fx["base"]))
        gen += int(fx["n_generated"])
        kept += fx["poses"].shape[0]
    return (gen - kept) / gen, gen - kept, gen


def generate(outdir, driver=None, asan_driver=None):
    """Writes every fixture into outdir.  asan_driver: the sanitizer build, which decides the exclusions (main() and the
    regeneration test pass it; without it nothing is screened)."""
    os.makedirs(outdir, exist_ok=True)
    fixtures = {}
    for c in cases():
        fx = run_case(c, driver, workdir=outdir, asan_driver=asan_driver)
        path = os.path.join(outdir, c["name"] + ".npz")
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (c["name"], size)
        fixtures[c["name"]] = refcase.load_fixture(path)
    return fixtures


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else refcase.GOLDEN_DIR
    assert refcase.reference_present(), "the reference tree is not here: " + refcase.REF
    refcase.build_driver()
    fixtures = generate(outdir, asan_driver=refcase.build_driver(asan=True))
    share, n_ex, n_gen = excluded_share(fixtures)
    print(f"excluded (reference undefined, shown by the sanitizer build): {n_ex} of {n_gen} start poses = {100 * share:.1f} %")
    assert share <= MAX_EXCLUDED_SHARE, share
    cov = coverage(fixtures)
    print("coverage:", cov)
    for name in sorted(fixtures):
        print(f"  {name}: {os.path.getsize(os.path.join(outdir, name + '.npz'))} bytes")
    codes = centroid_code_counts(fixtures)
    print("centroid codes 0..6 (legs fixtures):", codes)
    assert_coverage(cov, codes)


if __name__ == "__main__":
    main()
