"""The reference planner built on shims (oracle/_ref/ref_driver): case files, results, and what the oracle must say.

`tests/golden/make_ref_golden.py` and `tests/test_ref_golden.py` run the driver, which exists only where the reference
tree does.  `tests/test_gpu_ref_golden.py` uses only the fixture loaders of this module (load_fixture, fixture_names,
variant): it reads the committed fixtures and consults neither the driver nor the oracle.
A fixture stores its inputs (the map itself) and the REFERENCE's outputs; nothing in it comes from the oracle.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
REF = os.environ.get("REF", "/root/reference")
REF_SRC = os.path.join(REF, "foothold_planner", "src", "FootholdPlanner.cpp")
DRIVER = os.path.join(ORACLE_DIR, "_ref", "ref_driver")
DRIVER_ASAN = os.path.join(ORACLE_DIR, "_ref", "ref_driver_asan")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "ref")

H_REF = 0.01        # h_, cpp:336
DRIFT_REF = -0.007  # ajustedPose_[1] += -0.007, cpp:1578
OPT_REC = 49        # doubles per optimize() call in a service result, see parse_service

QUERY_DTYPE = np.dtype([("kind", "<i4"), ("cx", "<f8"), ("cy", "<f8"), ("foot_radius", "<f4"), ("search_radius", "<f4"),
                        ("vx", "<f8", (4,)), ("vy", "<f8", (4,))])
LEG_COLS = ("valid", "source", "x", "y", "z", "begin_row", "end_row", "no_map", "oob", "kind")
UNTOUCHED_ROW = -1000000


def reference_centroid_class(result):
    """What the REFERENCE's outputs alone say about each centroid query of a legs result (rows of other kinds: -1):
    6 the failed getSubmap (its ROS_ERROR, cpp:1629); 5 no result set and no such error; 0 a result set without a row
    scan (no read past the last column: the whole region was traversable); 1 a result set after a row scan (the oracle's
    codes 1-4: the reference reports which of its cases ran through stdout only)."""
    r = np.asarray(result)
    cls = np.full(r.shape[0], -1, np.int32)
    cen = r[:, 9] == 1
    untouched = np.isnan(r[:, 2])
    cls[cen & (r[:, 7] == 1)] = 6
    cls[cen & untouched & (r[:, 7] != 1)] = 5
    cls[cen & ~untouched & (r[:, 8] == 0)] = 0
    cls[cen & ~untouched & (r[:, 8] > 0)] = 1
    return cls


def load_fixture(path):
    """One tests/golden/ref/*.npz as a dict."""
    z = np.load(path)
    return {k: z[k] for k in z.files}


def fixture_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.endswith(".npz"))


def variant(fx, v):
    """The reference's outputs of one opt variant of a service fixture."""
    return {k[len(v) + 1:]: a for k, a in fx.items() if k.startswith(v + "/")}


def reference_present():
    return os.path.exists(REF_SRC)


def build_driver(asan=False):
    target = "_ref/ref_driver_asan" if asan else "_ref/ref_driver"
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, target, "REF=" + REF])
    return DRIVER_ASAN if asan else DRIVER


def _pstr(s):
    b = s.encode()
    return struct.pack("<i", len(b)) + b


def param_table(params, opt_params=None):
    """fpo.PARAMS_DTYPE (+ OPT_PARAMS_DTYPE) -> the reference's ROS parameter names (cpp:248-314); `global/*` are its
    file-scope constants (cpp:34-48).  h and lateralDrift are constants of the reference, not parameters."""
    p = np.asarray(params).reshape(1)[0]
    assert float(p["h"]) == H_REF and float(p["lateralDrift"]) == DRIFT_REF, "the reference fixes h_ and the lateral drift"
    t = {"debug": 0.0, "debug2": 0.0, "debug3": 0.0, "checkDefaultFoothold_Debug": 0.0,
         "footRadius": float(p["footRadius"]), "defaultFootholdThreshold": float(p["defaultFootholdThreshold"]),
         "candidateFootholdThreshold": float(p["candidateFootholdThreshold"]), "searchRadius": float(p["searchRadius"]),
         "stepLength": float(p["stepLength"]), "RF_FIRST": float(int(p["RF_FIRST"])),
         "laikago_kinematics/length": float(p["length"]), "laikago_kinematics/width": float(p["width"]),
         "laikago_kinematics/l1": float(p["l1"]), "laikago_kinematics/skewLength": float(p["skew"]),
         "nlopt/method": "LN_COBYLA"}
    if opt_params is not None:
        o = np.asarray(opt_params).reshape(1)[0]
        for k in ("w1", "w2", "w3", "w4", "wr", "wc"):
            t["nlopt/" + k] = float(o[k])
        t["nlopt/useInequalityConstraits"] = float(int(o["useInequalityConstraits"]))
        t["global/ctol"] = float(o["ctol"])
        t["global/hip_lower_scale"], t["global/hip_upper_scale"] = float(o["hipLowerScale"]), float(o["hipUpperScale"])
        t["global/skew_lower_scale"], t["global/skew_upper_scale"] = float(o["skewLowerScale"]), float(o["skewUpperScale"])
        t["global/lfCurrentRow"], t["global/rhCurrentRow"] = float(o["lfCurrentRow0"]), float(o["rhCurrentRow0"])
    return t


def write_case(path, mode, trav, elev, res, position, table, body):
    trav = np.ascontiguousarray(trav, np.float32)
    elev = np.ascontiguousarray(elev, np.float32)
    assert trav.shape == elev.shape and trav.ndim == 2
    with open(path, "wb") as f:
        f.write(b"FPREFC1\0")
        f.write(struct.pack("<iii", mode, trav.shape[0], trav.shape[1]))
        f.write(struct.pack("<ddd", float(res), float(position[0]), float(position[1])))
        f.write(trav.tobytes())
        f.write(elev.tobytes())
        f.write(struct.pack("<i", len(table)))
        for k, v in table.items():
            f.write(_pstr(k))
            if isinstance(v, str):
                f.write(struct.pack("<i", 1) + _pstr(v))
            else:
                f.write(struct.pack("<id", 0, float(v)))
        f.write(body)


def run_driver(case_path, driver=None, timeout=600):
    """Run one case; returns the flat f64 result.  HOME points at a scratch directory under oracle/_ref/."""
    driver = driver or DRIVER
    home = os.path.join(ORACLE_DIR, "_ref", "home")
    os.makedirs(home, exist_ok=True)
    out = case_path + ".out"
    env = dict(os.environ, HOME=home)
    r = subprocess.run([driver, case_path, out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{os.path.basename(driver)} exit {r.returncode}: {r.stderr.decode(errors='replace')[-4000:]}")
    return np.fromfile(out, np.float64)


def legs_body(queries):
    q = np.ascontiguousarray(queries, QUERY_DTYPE)
    return struct.pack("<i", q.shape[0]) + q.tobytes()


def service_body(poses, n_cycles):
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    b = struct.pack("<i", poses.shape[0])
    for x, y, z in poses:
        b += struct.pack("<dddi", x, y, z, int(n_cycles))
    return b


def parse_legs(flat, n):
    return flat.reshape(n, len(LEG_COLS))


def parse_service(flat, B, N):
    """-> dict of padded arrays, one row per start pose.  Tracks: (N+1)*4 footholds at most."""
    M = (N + 1) * 4
    o = {"ret": np.zeros(B, np.uint8), "fail_cycle": np.full(B, 255, np.uint8), "oob": np.zeros(B, np.int64),
         "response_n": np.zeros(B, np.int32), "opt_n": np.zeros(B, np.int32), "opt_rec": np.zeros((B, N, OPT_REC))}
    for t in ("nominal", "centroid", "opt"):
        o[t + "_head"] = np.zeros((B, 5), np.int32)  # published, success, gait_cycles, gait_cycles_succeed, n footholds
        o[t + "_id"] = np.zeros((B, M, 2), np.uint8)  # foot_id, gait_cycle_id
        o[t + "_xyz"] = np.zeros((B, M, 3))
    o["nominal_path_n"], o["centroid_path_n"] = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    o["nominal_path"], o["centroid_path"] = np.zeros((B, N, 3)), np.zeros((B, 2 * N, 3))
    at = 0

    def take(k):
        nonlocal at
        v = flat[at:at + k]
        assert v.size == k, "driver result truncated"
        at += k
        return v

    for b in range(B):
        ret, gates, oob, nresp = take(4)
        o["ret"][b], o["oob"][b], o["response_n"][b] = int(ret), int(oob), int(nresp)
        if not ret:
            o["fail_cycle"][b] = int(gates)
        for t in ("nominal", "centroid", "opt"):
            npub = int(take(1)[0])
            if npub:
                succ, gc, gcs, nf = (int(v) for v in take(4))
                o[t + "_head"][b] = (npub > 0, succ, gc, gcs, nf)
                rec = take(5 * nf).reshape(nf, 5)
                o[t + "_id"][b, :nf] = rec[:, :2]
                o[t + "_xyz"][b, :nf] = rec[:, 2:]
        for t in ("nominal_path", "centroid_path"):
            if int(take(1)[0]):
                n = int(take(1)[0])
                o[t + "_n"][b] = n
                o[t][b, :n] = take(3 * n).reshape(n, 3)
        n = int(take(1)[0])
        o["opt_n"][b] = n
        o["opt_rec"][b, :n] = take(OPT_REC * n).reshape(n, OPT_REC)
    assert at == flat.size, (at, flat.size)
    return o


def run_service(trav, elev, res, position, params, opt_params, poses, n_cycles, driver=None, workdir=None):
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    with tempfile.TemporaryDirectory(dir=workdir) as d:
        case = os.path.join(d, "case.bin")
        write_case(case, 1, trav, elev, res, position, param_table(params, opt_params), service_body(poses, n_cycles))
        return parse_service(run_driver(case, driver), poses.shape[0], n_cycles)


def run_legs(trav, elev, res, position, params, queries, driver=None, workdir=None):
    with tempfile.TemporaryDirectory(dir=workdir) as d:
        case = os.path.join(d, "case.bin")
        write_case(case, 0, trav, elev, res, position, param_table(params), legs_body(queries))
        return parse_legs(run_driver(case, driver), len(queries))


# ---- what the ORACLE says about the same inputs, laid out as the reference's outputs are ------------------------------

def _bits(a):
    a = np.ascontiguousarray(a, np.float64)
    return a.view(np.uint64)


def assert_same(ref, ora, what):
    """Bit-exact: integers equal, doubles the same bits (NaN payloads aside: NaN == NaN)."""
    ref, ora = np.asarray(ref), np.asarray(ora)
    assert ref.shape == ora.shape, f"{what}: shape {ref.shape} vs {ora.shape}"
    if ref.dtype.kind == "f" or ora.dtype.kind == "f":
        r, q = np.asarray(ref, np.float64), np.asarray(ora, np.float64)
        bad = ~((_bits(r) == _bits(q)) | (np.isnan(r) & np.isnan(q)) | ((r == 0) & (q == 0)))
    else:
        bad = ref != ora
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {i}: reference {ref[i]!r} oracle {ora[i]!r}")


def oracle_service(omap, params, opt_params, poses, N):
    """The oracle's plan, opt track and products for the poses, in the layout of parse_service."""
    from oracle import fpo
    from tests.conftest import oracle_poses

    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    B = poses.shape[0]
    op = oracle_poses(poses)
    plan = omap.plan(params, op, N)
    opt = omap.plan_opt(params, opt_params, op, N, plan["cycle_ok"])
    M = (N + 1) * 4
    o = {"ret": (opt["gate_fail_cycle"] == 255).astype(np.uint8), "fail_cycle": opt["gate_fail_cycle"].astype(np.uint8),
         "opt_n": np.zeros(B, np.int32), "opt_rec": np.zeros((B, N, OPT_REC)), "plan": plan, "opt": opt}
    for t in ("nominal", "centroid", "opt"):
        o[t + "_head"] = np.zeros((B, 5), np.int32)
        o[t + "_id"] = np.zeros((B, M, 2), np.uint8)
        o[t + "_xyz"] = np.zeros((B, M, 3))
    o["nominal_path_n"], o["centroid_path_n"] = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    o["nominal_path"], o["centroid_path"] = np.zeros((B, N, 3)), np.zeros((B, 2 * N, 3))
    o["response_n"] = np.zeros(B, np.int32)
    for b in range(B):
        gate = int(opt["gate_fail_cycle"][b])
        ncyc = N if gate == 255 else gate
        o["opt_n"][b] = ncyc
        c = opt["cycles"][b]
        for g in range(ncyc):
            o["opt_rec"][b, g] = np.concatenate([
                c["gait_top_left"][g], c["gait_size"][g], c["nominal_index"][g], c["centroid_index"][g], c["x_lower"][g],
                c["x_upper"][g], c["x"][g], [c["minf"][g], c["lf_current_row"][g], c["rh_current_row"][g], c["solver_status"][g],
                                             8 * int(np.asarray(opt_params).reshape(1)[0]["useInequalityConstraits"])]])
        ok = plan["cycle_ok"][b].astype(bool)
        committed = np.nonzero(ok[:ncyc])[0]  # a refused call (the handler returned false in cycle `gate`) ran the cycles before
        last = int(committed[-1]) if committed.size else -1
        if last >= 0:  # the paths are published on commit (cpp:1410, 1477) and hold every cycle planned so far
            pr = omap.plan_products(params, op[b:b + 1], N)
            po = omap.plan_opt_products(params, opt_params, op[b:b + 1], N, plan["cycle_ok"][b])
            o["nominal_path_n"][b] = last + 1
            o["nominal_path"][b, :last + 1] = pr["nominal"]["path"][:last + 1]
            o["centroid_path_n"][b] = 2 * (last + 1)
            inter = np.zeros((2 * (last + 1), 3))
            inter[0::2] = pr["centroid"]["path"][:last + 1]  # the centroid track's push (cpp:792) ...
            inter[1::2] = po["path"][:last + 1]              # ... and the opt track's onto the SAME path (cpp:946)
            o["centroid_path"][b, :2 * (last + 1)] = inter
        if gate != 255:
            continue  # the handler returned false (cpp:931-934): no GlobalFootholds message, no response
        src = {"nominal": plan["nominal"][b], "centroid": plan["centroid"][b], "opt": opt["footholds"][b]}
        for t in ("nominal", "centroid", "opt"):
            ids, xyz = [], []
            for l in range(4):  # the initial stance, gait_cycle_id 0 (cpp:681-755)
                ids.append((l, 0))
                xyz.append(plan["stance"][b, l])
            for g in committed:
                for l in range(4):
                    ids.append((l, g))
                    xyz.append((src[t]["x"][g, l], src[t]["y"][g, l], float(src[t]["z"][g, l])))
            nf = len(ids)
            # success: set true by a commit; ONLY the nominal message is set false again by a failed cycle (cpp:1574)
            succ = int(committed.size > 0 and (t != "nominal" or bool(ok[-1]))) if N > 0 else 0
            o[t + "_head"][b] = (1, succ, N if t == "nominal" else 0, last + 1, nf)
            o[t + "_id"][b, :nf] = ids
            o[t + "_xyz"][b, :nf] = xyz
        o["response_n"][b] = o["nominal_head"][b, 4]
    return o


SERVICE_KEYS = ("ret", "fail_cycle", "response_n", "nominal_head", "nominal_id", "nominal_xyz", "centroid_head", "centroid_id",
                "centroid_xyz", "opt_head", "opt_id", "opt_xyz", "nominal_path_n", "nominal_path", "centroid_path_n",
                "centroid_path", "opt_n", "opt_rec")


def assert_service_equal(ref, ora, what=""):
    for k in SERVICE_KEYS:
        assert_same(ref[k], ora[k], f"{what}{k}")


def oracle_legs(omap, params, queries):
    """-> array [n, 7]: valid, source, x, y, z, begin_row, end_row as the reference reports them (see ref_driver.cpp),
    plus the oracle's centroid codes (label only)."""
    from oracle import fpo

    q = np.asarray(queries, QUERY_DTYPE)
    out = np.zeros((q.shape[0], 8))
    codes = np.full(q.shape[0], -1, np.int32)
    p = np.array(params, dtype=fpo.PARAMS_DTYPE).reshape(1)
    for k, r in enumerate(q):
        if r["kind"] == 0:
            pq = p.copy()
            pq["footRadius"] = r["foot_radius"]
            oq = np.zeros(1, fpo.QUERY_DTYPE)
            oq["cx"], oq["cy"], oq["search_radius"], oq["n_vertices"] = r["cx"], r["cy"], r["search_radius"], 4
            oq["vx"][0, :4], oq["vy"][0, :4] = r["vx"], r["vy"]
            leg = omap.search_legs(pq, oq)[0]
            out[k, :5] = (leg["valid"], leg["source"], leg["x"], leg["y"], float(leg["z"]))
        elif r["kind"] == 1:
            c, code, begin, end = omap.centroid_rows(p, float(r["cx"]), float(r["cy"]), float(p["searchRadius"][0]))
            codes[k] = code
            if code >= 5:
                out[k, 2:7] = (np.nan, np.nan, np.nan, UNTOUCHED_ROW, UNTOUCHED_ROW)
            else:
                out[k, 2:7] = (c["x"], c["y"], float(c["z"]), begin, end)
            out[k, 7] = code == 6
        else:
            out[k, 4] = omap.mean_height(float(r["cx"]), float(r["cy"]), float(r["foot_radius"]), H_REF)
    return out, codes


def assert_legs_equal(ref, ora, what=""):
    for k, name in enumerate(LEG_COLS[:8]):
        assert_same(ref[:, k], ora[:, k], f"{what}{name}")
