"""ORACLE — TEST INFRASTRUCTURE ONLY.  Parity with the reference: pinned for the logic of FootholdPlanner.cpp by
tests/golden/ref/ (the reference's own planner built on shims, oracle/ref_shim/); grid_map_core's semantics stay unpinned
(see oracle/fpo_gridmap.hpp).

ctypes loader for the CPU restatement (oracle/_build/libfpo.so).  Only tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module; the engine
(quadrupedal_foothold_planner_amd/) never does.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "libfpo.so")

# numpy mirrors of the C records in fpo_capi.cpp / fpo_planner.hpp
PARAMS_DTYPE = np.dtype(
    [
        ("footRadius", "<f4"),
        ("defaultFootholdThreshold", "<f4"),
        ("candidateFootholdThreshold", "<f4"),
        ("searchRadius", "<f4"),
        ("stepLength", "<f4"),
        ("length", "<f4"),
        ("width", "<f4"),
        ("l1", "<f4"),
        ("skew", "<f4"),
        ("RF_FIRST", "<i4"),
        ("h", "<f8"),
        ("lateralDrift", "<f8"),
    ],
    align=True,
)
POSE_DTYPE = np.dtype(
    [("pose", "<f8", (3,)), ("gait", "<i4"), ("legRadius", "<f4", (4,)), ("legPoly", "<i4", (4,))],
    align=True,
)
LEG_DTYPE = np.dtype(
    [("row", "<i4"), ("col", "<i4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f4"), ("valid", "u1"), ("source", "u1"), ("pad", "u1", (2,))],
    align=True,
)
CENTROID_DTYPE = np.dtype(
    [("x", "<f8"), ("y", "<f8"), ("z", "<f4"), ("row", "<i4"), ("col", "<i4"), ("code", "u1"), ("pad", "u1", (3,))],
    align=True,
)
QUERY_DTYPE = np.dtype(
    [("cx", "<f8"), ("cy", "<f8"), ("search_radius", "<f4"), ("n_vertices", "<i4"), ("vx", "<f8", (8,)), ("vy", "<f8", (8,))],
    align=True,
)

# fpo_opt.cpp: OptParams / the per-cycle record and the per-leg result of the opt track; the two record
# layouts are the engine's fpe_opt_cycle / fpe_opt_foothold (include/fpe.h)
OPT_PARAMS_DTYPE = np.dtype(
    [("w1", "<f8"), ("w2", "<f8"), ("w3", "<f8"), ("w4", "<f8"), ("wr", "<f8"), ("wc", "<f8"),
     ("useInequalityConstraits", "<i4"), ("pad", "<i4"), ("ctol", "<f8"),
     ("hipLowerScale", "<f8"), ("hipUpperScale", "<f8"), ("skewLowerScale", "<f8"), ("skewUpperScale", "<f8"),
     ("lfCurrentRow0", "<f8"), ("rhCurrentRow0", "<f8")],
    align=True,
)
OPT_FOOTHOLD_DTYPE = np.dtype(
    [("x", "<f8"), ("y", "<f8"), ("z", "<f4"), ("row", "<i4"), ("col", "<i4"), ("foot_id", "u1"), ("gait_cycle_id", "u1"),
     ("committed", "u1"), ("pad", "u1")],
    align=True,
)
OPT_CYCLE_DTYPE = np.dtype(
    [("gait_top_left", "<i4", (2,)), ("gait_size", "<i4", (2,)), ("nominal_index", "<i4", (8,)), ("centroid_index", "<i4", (8,)),
     ("traversable_row", "<i4", (2, 4)), ("x_lower", "<i4", (8,)), ("x_upper", "<i4", (8,)), ("x", "<i4", (8,)),
     ("minf", "<f8"), ("lf_current_row", "<f8"), ("rh_current_row", "<f8"), ("centroid_code", "u1", (4,)),
     ("gate_failed", "u1"), ("committed", "u1"), ("solver_status", "u1"), ("pad", "u1")],
    align=True,
)


def opt_params_yaml():
    """nlopt/* of foothold_planner.yaml:53-63 plus the file-scope constants of FootholdPlanner.cpp:28-51."""
    op = np.zeros(1, OPT_PARAMS_DTYPE)
    for k in ("w1", "w2", "w3", "w4", "wr", "wc"):
        op[k] = 1.0
    op["useInequalityConstraits"] = 1
    op["ctol"] = 1e-2
    op["hipLowerScale"], op["hipUpperScale"] = 0.9, 1.1
    op["skewLowerScale"], op["skewUpperScale"] = 0.8, 1.2
    return op


# fpo_filters.cpp: FilterParams (the producer's default chain)
FILTER_PARAMS_DTYPE = np.dtype(
    [
        ("normalRadius", "<f8"),
        ("slopeCritical", "<f8"),
        ("stepCritical", "<f8"),
        ("stepFirstRadius", "<f8"),
        ("stepSecondRadius", "<f8"),
        ("stepCriticalCells", "<i4"),
        ("pad", "<i4"),
        ("roughnessCritical", "<f8"),
        ("roughnessRadius", "<f8"),
    ],
    align=True,
)
FILTER_LAYERS = ("normal_x", "normal_y", "normal_z", "slope", "step_height", "step", "roughness", "traversability")


class _Map(C.Structure):
    _fields_ = [
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("resolution", C.c_double),
        ("position", C.c_double * 2),
        ("traversability", C.c_void_p),
        ("elevation", C.c_void_p),
        ("row_major", C.c_int32),
    ]


def build(force=False):
    """Compile the oracle with the committed Makefile (g++, -ffp-contract=off) and, where the reference tree is present,
    the reference driver (build_reference_driver)."""
    _build_lib(force)
    build_reference_driver()
    return _LIB_PATH


def _build_lib(force=False):
    if force or not os.path.exists(_LIB_PATH) or any(
        os.path.getmtime(os.path.join(_HERE, f)) > os.path.getmtime(_LIB_PATH)
        for f in ("fpo_gridmap.hpp", "fpo_planner.hpp", "fpo_planner.cpp", "fpo_opt.cpp", "fpo_capi.cpp", "fpo_filters.cpp", "Makefile")
    ):
        subprocess.check_call(["make", "-s", "-C", _HERE])
    return _LIB_PATH


REF = os.environ.get("REF", "/root/reference")
REF_DRIVER = os.path.join(_HERE, "_ref", "ref_driver")
REF_DRIVER_STATUS = ""


def build_reference_driver():
    """oracle/_ref/ref_driver: the REFERENCE's own FootholdPlanner.cpp compiled verbatim, in place, against the shim headers
    of oracle/ref_shim/ (Makefile target _ref/ref_driver; make rebuilds it when a shim, the driver or the reference is
    newer).  Only where the reference tree is present; says in one line what it did."""
    global REF_DRIVER_STATUS
    src = os.path.join(REF, "foothold_planner", "src", "FootholdPlanner.cpp")
    if not os.path.exists(src):
        REF_DRIVER_STATUS = f"oracle/_ref/ref_driver skipped: no reference tree at {REF}"
    else:
        subprocess.check_call(["make", "-s", "-C", _HERE, "_ref/ref_driver", "REF=" + REF])
        REF_DRIVER_STATUS = f"oracle/_ref/ref_driver built from the reference in place ({src})"
    print("build:", REF_DRIVER_STATUS)
    return REF_DRIVER_STATUS


_lib = None


def lib():
    global _lib
    if _lib is None:
        _build_lib()
        L = C.CDLL(_LIB_PATH)
        L.fpo_map_create.restype = C.c_void_p
        L.fpo_map_create.argtypes = [C.POINTER(_Map)]
        L.fpo_map_destroy.argtypes = [C.c_void_p]
        L.fpo_plan.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.fpo_search_legs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.fpo_pose_status.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.fpo_gate_lateral.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.fpo_plan_as_written.restype = C.c_ulonglong
        L.fpo_plan_as_written.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.fpo_plan_products.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.fpo_centroid_method.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_float, C.c_void_p]
        L.fpo_mean_height.restype = C.c_float
        L.fpo_mean_height.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_float, C.c_double]
        L.fpo_spiral_cells.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int]
        L.fpo_circle_cells.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int]
        L.fpo_get_index.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        L.fpo_get_position.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.fpo_submap_info.argtypes = [C.c_void_p] + [C.c_double] * 4 + [C.c_void_p, C.c_void_p]
        L.fpo_polygon_inside.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double]
        L.fpo_polygon_center.argtypes = [C.c_void_p, C.c_void_p]
        L.fpo_constants.argtypes = [C.c_void_p, C.c_void_p]
        L.fpo_plan_opt.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 4
        L.fpo_plan_opt_products.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5
        L.fpo_solve_lattice.argtypes = [C.c_void_p] * 5 + [C.c_double] * 5 + [C.c_void_p] * 2
        L.fpo_plan_opt_forced.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.fpo_centroid_on_submap.argtypes = [C.c_void_p, C.c_void_p] + [C.c_double] * 6 + [C.c_float, C.c_void_p, C.c_void_p]
        L.fpo_centroid_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_float, C.c_void_p, C.c_void_p]
        L.fpo_filter_defaults.argtypes = [C.c_void_p]
        L.fpo_filters.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.fpo_sizeof(0) == PARAMS_DTYPE.itemsize
        assert L.fpo_sizeof(1) == POSE_DTYPE.itemsize
        assert L.fpo_sizeof(2) == LEG_DTYPE.itemsize
        assert L.fpo_sizeof(3) == CENTROID_DTYPE.itemsize
        assert L.fpo_sizeof(4) == QUERY_DTYPE.itemsize
        assert L.fpo_sizeof(5) == C.sizeof(_Map)
        assert L.fpo_sizeof(6) == OPT_PARAMS_DTYPE.itemsize
        assert L.fpo_sizeof(7) == OPT_FOOTHOLD_DTYPE.itemsize == 32
        assert L.fpo_sizeof(8) == OPT_CYCLE_DTYPE.itemsize == 240
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class OracleMap:
    """A canonical (start index 0) grid map: row-major (rows, cols) f32 layers, f64 geometry."""

    def __init__(self, traversability, elevation, resolution, position=(0.0, 0.0)):
        self.trav = np.ascontiguousarray(traversability, dtype=np.float32)
        self.elev = np.ascontiguousarray(elevation, dtype=np.float32)
        assert self.trav.shape == self.elev.shape and self.trav.ndim == 2
        self.rows, self.cols = self.trav.shape
        self.resolution = float(resolution)
        self.position = (float(position[0]), float(position[1]))
        m = _Map(self.rows, self.cols, self.resolution, (C.c_double * 2)(*self.position), _ptr(self.trav), _ptr(self.elev), 1)
        self._h = lib().fpo_map_create(C.byref(m))

    def __del__(self):
        try:
            if self._h:
                lib().fpo_map_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- chained plan -------------------------------------------------------------------------
    def plan(self, params, poses, n_cycles, threads=1, out=None):
        """params: PARAMS_DTYPE scalar array; poses: POSE_DTYPE array [B].  `out` may be a dict of
        preallocated arrays from a previous call (timing loops reuse it)."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        if out is None:
            out = {
                "nominal": np.zeros((B, n_cycles, 4), dtype=LEG_DTYPE),
                "centroid": np.zeros((B, n_cycles, 4), dtype=CENTROID_DTYPE),
                "default": np.zeros((B, n_cycles, 4, 3), dtype=np.float64),
                "cycle_ok": np.zeros((B, n_cycles), dtype=np.uint8),
                "stance": np.zeros((B, 4, 3), dtype=np.float64),
            }
        rc = lib().fpo_plan(self._h, _ptr(params), _ptr(poses), B, n_cycles, threads, _ptr(out["nominal"]),
                            _ptr(out["centroid"]), _ptr(out["default"]), _ptr(out["cycle_ok"]), _ptr(out["stance"]))
        assert rc == 0
        return out

    def pose_status(self, params, poses):
        """bit 0 per pose: getGaitCycleSearchGridMap fails in the first gait cycle (the service returns false, cpp:931-934)."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        out = np.zeros(poses.shape[0], dtype=np.uint8)
        lib().fpo_pose_status(self._h, _ptr(params), _ptr(poses), poses.shape[0], _ptr(out))
        return out

    def gate_lateral(self, params, poses, n_cycles):
        """First gait cycle whose getGaitCycleSearchGridMap fails on its LATERAL (y) side, per pose; 255 = none: the
        optimiser-independent part of the handler's gate in every cycle (fpo_capi.cpp::fpo_gate_lateral)."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        out = np.zeros(poses.shape[0], dtype=np.uint8)
        lib().fpo_gate_lateral(self._h, _ptr(params), _ptr(poses), poses.shape[0], int(n_cycles), _ptr(out))
        return out

    def plan_as_written(self, params, poses, n_cycles):
        """Same results as plan(); additionally performs the reference's by-value whole-map copies
        (cost emulation, see fpo_planner.hpp).  Returns (nominal, number_of_map_copies)."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        nominal = np.zeros((poses.shape[0], n_cycles, 4), dtype=LEG_DTYPE)
        n = lib().fpo_plan_as_written(self._h, _ptr(params), _ptr(poses), poses.shape[0], n_cycles, _ptr(nominal))
        return nominal, int(n)

    def plan_products(self, params, pose, n_cycles):
        """Feet-centre paths and KPIs of one trot plan: {"centroid"|"nominal": {"path", "feet_distance", "cog_speed"}}."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        pose = np.ascontiguousarray(pose, dtype=POSE_DTYPE).reshape(1)
        n = max(int(n_cycles), 1)
        path = [np.zeros((n, 3)), np.zeros((n, 3))]
        dist = [np.zeros(2 * n), np.zeros(2 * n)]
        speed = [np.zeros(2 * n), np.zeros(2 * n)]
        counts = np.zeros(4, dtype=np.int32)
        lib().fpo_plan_products(self._h, _ptr(params), _ptr(pose), int(n_cycles), _ptr(path[0]), _ptr(path[1]), _ptr(dist[0]),
                                _ptr(dist[1]), _ptr(speed[0]), _ptr(speed[1]), _ptr(counts))
        out = {}
        for k, name in enumerate(("centroid", "nominal")):
            out[name] = {"path": path[k][: counts[2 * k]].copy(), "feet_distance": dist[k][: counts[2 * k + 1]].copy(),
                         "cog_speed": speed[k][: counts[2 * k + 1]].copy()}
        return out

    # ---- the opt track ---------------------------------------------------------
    def plan_opt(self, params, opt_params, poses, n_cycles, cycle_ok):
        """cycle_ok: [B, n_cycles] of the nominal plan.  Returns {"footholds" [B, n, 4], "cycles" [B, n], "gate_fail_cycle" [B]}."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        op = np.ascontiguousarray(opt_params, dtype=OPT_PARAMS_DTYPE).reshape(1)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        ok = np.ascontiguousarray(cycle_ok, dtype=np.uint8).reshape(B, n_cycles)
        out = {"footholds": np.zeros((B, n_cycles, 4), OPT_FOOTHOLD_DTYPE), "cycles": np.zeros((B, n_cycles), OPT_CYCLE_DTYPE),
               "gate_fail_cycle": np.zeros(B, np.uint8)}
        rc = lib().fpo_plan_opt(self._h, _ptr(params), _ptr(op), _ptr(poses), B, n_cycles, _ptr(ok), _ptr(out["footholds"]),
                                _ptr(out["cycles"]), _ptr(out["gate_fail_cycle"]))
        assert rc == 0
        return out

    def plan_opt_forced(self, params, opt_params, pose, n_cycles, cycle_ok, forced_x):
        """One pose's opt track with the optimiser's x of the first len(forced_x) cycles SUPPLIED (doubles, [k, 8]): the cycles'
        records and the gate verdict (255: none).  An external optimiser drives the literal chain (make_cobyla_golden.py)."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        op = np.ascontiguousarray(opt_params, dtype=OPT_PARAMS_DTYPE).reshape(1)
        pose = np.ascontiguousarray(pose, dtype=POSE_DTYPE).reshape(1)
        ok = np.ascontiguousarray(cycle_ok, dtype=np.uint8).reshape(n_cycles)
        fx = np.ascontiguousarray(forced_x, dtype=np.float64).reshape(-1, 8) if len(forced_x) else np.zeros((0, 8))
        cycles = np.zeros(n_cycles, OPT_CYCLE_DTYPE)
        gate = np.zeros(1, np.int32)
        rc = lib().fpo_plan_opt_forced(self._h, _ptr(params), _ptr(op), _ptr(pose), int(n_cycles), _ptr(ok), _ptr(fx) if fx.size else None,
                                       int(fx.shape[0]), _ptr(cycles), _ptr(gate))
        assert rc == 0
        return cycles, (255 if gate[0] < 0 else int(gate[0]))

    def plan_opt_products(self, params, opt_params, pose, n_cycles, cycle_ok):
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        op = np.ascontiguousarray(opt_params, dtype=OPT_PARAMS_DTYPE).reshape(1)
        pose = np.ascontiguousarray(pose, dtype=POSE_DTYPE).reshape(1)
        ok = np.ascontiguousarray(cycle_ok, dtype=np.uint8).reshape(n_cycles)
        n = max(int(n_cycles), 1)
        path, dist, speed, counts = np.zeros((n, 3)), np.zeros(2 * n), np.zeros(2 * n), np.zeros(3, np.int32)
        lib().fpo_plan_opt_products(self._h, _ptr(params), _ptr(op), _ptr(pose), int(n_cycles), _ptr(ok), _ptr(path), _ptr(dist),
                                    _ptr(speed), _ptr(counts))
        return {"path": path[: counts[0]].copy(), "feet_distance": dist[: counts[1]].copy(), "cog_speed": speed[: counts[1]].copy(),
                "gate_fail_cycle": int(counts[2])}

    def centroid_on_submap(self, params, sub_centre, sub_length, x, y, search_radius):
        """checkFootholdUseCentroidMethod on getSubmap(sub_centre, sub_length) of this map (the opt track's use)."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        out = np.zeros(1, dtype=CENTROID_DTYPE)
        o6 = np.zeros(6, dtype=np.int32)
        ok = lib().fpo_centroid_on_submap(self._h, _ptr(params), sub_centre[0], sub_centre[1], sub_length[0], sub_length[1], x, y,
                                          search_radius, _ptr(out), _ptr(o6))
        return bool(ok), out[0], {"code": int(o6[0]), "begin_row": int(o6[1]), "end_row": int(o6[2]), "row": int(o6[3]), "col": int(o6[4])}

    def search_legs(self, params, queries):
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        queries = np.ascontiguousarray(queries, dtype=QUERY_DTYPE)
        out = np.zeros(queries.shape[0], dtype=LEG_DTYPE)
        lib().fpo_search_legs(self._h, _ptr(params), _ptr(queries), queries.shape[0], _ptr(out))
        return out

    def centroid_method(self, params, x, y, search_radius):
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        out = np.zeros(1, dtype=CENTROID_DTYPE)
        lib().fpo_centroid_method(self._h, _ptr(params), x, y, search_radius, _ptr(out))
        return out[0]

    def centroid_rows(self, params, x, y, search_radius):
        """checkFootholdUseCentroidMethod on this map with the band's rows: (record, code, begin_row, end_row)."""
        params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
        out = np.zeros(1, dtype=CENTROID_DTYPE)
        o3 = np.zeros(3, dtype=np.int32)
        lib().fpo_centroid_rows(self._h, _ptr(params), x, y, search_radius, _ptr(out), _ptr(o3))
        return out[0], int(o3[0]), int(o3[1]), int(o3[2])

    def mean_height(self, x, y, radius, h=0.01):
        return float(lib().fpo_mean_height(self._h, x, y, np.float32(radius), h))

    # ---- grid_map probes ------------------------------------------------------------------------
    def spiral_cells(self, cx, cy, radius, max_cells=1 << 16):
        buf = np.zeros((max_cells, 2), dtype=np.int32)
        n = lib().fpo_spiral_cells(self._h, cx, cy, radius, _ptr(buf), max_cells)
        return buf[:n].copy()

    def circle_cells(self, cx, cy, radius, max_cells=1 << 16):
        buf = np.zeros((max_cells, 2), dtype=np.int32)
        n = lib().fpo_circle_cells(self._h, cx, cy, radius, _ptr(buf), max_cells)
        return buf[:n].copy()

    def get_index(self, x, y):
        ij = np.zeros(2, dtype=np.int32)
        ok = lib().fpo_get_index(self._h, x, y, _ptr(ij))
        return bool(ok), int(ij[0]), int(ij[1])

    def get_position(self, i, j):
        xy = np.zeros(2, dtype=np.float64)
        ok = lib().fpo_get_position(self._h, i, j, _ptr(xy))
        return bool(ok), float(xy[0]), float(xy[1])

    def submap_info(self, x, y, lx, ly):
        o = np.zeros(4, dtype=np.int32)
        pl = np.zeros(4, dtype=np.float64)
        ok = lib().fpo_submap_info(self._h, x, y, lx, ly, _ptr(o), _ptr(pl))
        return bool(ok), o, pl


def solve_lattice(opt_params, nominal_index, centroid_index, lo, up, length_base, skew, resolution, lf_row=0.0, rh_row=0.0):
    """The build-defined optimiser of the opt track alone: returns (status, x[8], minf)."""
    op = np.ascontiguousarray(opt_params, dtype=OPT_PARAMS_DTYPE).reshape(1)
    a = [np.ascontiguousarray(v, dtype=np.int32).reshape(8) for v in (nominal_index, centroid_index, lo, up)]
    x, minf = np.zeros(8), np.zeros(1)
    st = lib().fpo_solve_lattice(_ptr(op), _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), float(length_base), float(skew),
                                 float(resolution), float(lf_row), float(rh_row), _ptr(x), _ptr(minf))
    return int(st), x, float(minf[0])


def polygon_inside(vx, vy, x, y):
    vx = np.ascontiguousarray(vx, dtype=np.float64)
    vy = np.ascontiguousarray(vy, dtype=np.float64)
    return bool(lib().fpo_polygon_inside(_ptr(vx), _ptr(vy), len(vx), x, y))


def polygon_center(feet):
    feet = np.ascontiguousarray(feet, dtype=np.float64).reshape(12)
    out = np.zeros(3, dtype=np.float64)
    lib().fpo_polygon_center(_ptr(feet), _ptr(out))
    return out


def constants(params):
    params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
    out = np.zeros(14, dtype=np.float64)
    lib().fpo_constants(_ptr(params), _ptr(out))
    return {"LbHalf": out[0], "WbHalfNeg": out[1], "WbHalfPos": out[2], "biasX": out[3:7].copy(),
            "biasY": out[7:11].copy(), "stepHalf": out[11], "step": out[12], "stepQuarter": out[13]}


def filter_defaults():
    fp = np.zeros(1, FILTER_PARAMS_DTYPE)
    assert lib().fpo_filter_defaults(_ptr(fp)) == 0
    return fp


def traversability_filters(elevation, resolution, position=(0.0, 0.0), params=None):
    """elevation: rows x cols float32 (row-major numpy, start index 0) -> dict of the eight layers, same shape."""
    elev = np.asarray(elevation, np.float32)
    rows, cols = elev.shape
    fp = filter_defaults() if params is None else params
    src = np.asfortranarray(elev)  # grid_map::Matrix is column-major
    out = np.empty((8, cols, rows), np.float32)  # each layer column-major = the transpose, row-major
    rc = lib().fpo_filters(rows, cols, float(resolution), float(position[0]), float(position[1]),
                           src.ctypes.data_as(C.c_void_p), _ptr(fp), _ptr(out))
    assert rc == 0
    return {name: np.ascontiguousarray(out[k].T) for k, name in enumerate(FILTER_LAYERS)}
