"""ctypes binding of libfpe.so (include/fpe.h).  Every struct of the header has ONE written-out mirror here — a numpy structured
dtype for the records that live in arrays, a ctypes.Structure for what is passed by reference, the second form derived from the
first where both are needed — and STRUCTS names them all; PROTOTYPES holds every entry point's restype and argtypes.
tests/test_cpu_abi.py compares size, every field's offset and size, and the field tiling of each mirror with the C compiler's."""
import ctypes as C
import os

import numpy as np

from . import build as _build

FPE_OK = 0
FPE_E_INVALID_ARG = -1
FPE_E_NO_MAP = -2
FPE_E_HIP = -3
FPE_E_NO_DEVICE = -4
FPE_E_UNSUPPORTED = -5
FPE_E_NOMEM = -6
FPE_E_SERVICE_FALSE = -7
FPE_POSE_OPT_SUBMAP_FAILED = 1

MAX_POLYGON_VERTICES = 8

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
    [("position", "<f8", (3,)), ("gait", "<i4"), ("leg_search_radius", "<f4", (4,)), ("leg_polygon_kind", "<i4", (4,))],
    align=True,
)
FOOTHOLD_DTYPE = np.dtype(
    [("row", "<i4"), ("col", "<i4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f4"), ("valid", "u1"), ("source", "u1"),
     ("foot_id", "u1"), ("gait_cycle_id", "u1")],
    align=True,
)
CENTROID_DTYPE = np.dtype(
    [("x", "<f8"), ("y", "<f8"), ("z", "<f4"), ("row", "<i4"), ("col", "<i4"), ("code", "u1"), ("pad", "u1", (3,))],
    align=True,
)
# fpe_stride: step length and lateral drift of ONE pose (fpe_plan_strides*, fpe_plan_rank_strides*); element b belongs to poses[b]
STRIDE_DTYPE = np.dtype([("step_length", "<f4"), ("reserved", "<i4"), ("lateral_drift", "<f8")], align=True)
# fpe_plan_state: the state of ONE pose's chain between two gait cycles (fpe_plan_resume*): feet[track][leg][x, y], the running
# lateral drift and the number of cycles planned so far
PLAN_STATE_DTYPE = np.dtype([("feet", "<f8", (3, 4, 2)), ("adjusted_y", "<f8"), ("cycle", "<i4"), ("reserved", "<i4")], align=True)
# fpe_selected_foothold: the 16-byte multi-GPU exchange record
SELECTED_DTYPE = np.dtype(
    [("row", "<i4"), ("col", "<i4"), ("z", "<f4"), ("valid", "u1"), ("source", "u1"), ("foot_id", "u1"), ("gait_cycle_id", "u1")],
    align=True,
)
# fpe_selected_packed: the 8-byte exchange record ((row + 256) | (col + 256) << 14 | valid << 28 | source << 29, z)
PACKED_DTYPE = np.dtype([("cell", "<u4"), ("z", "<f4")], align=True)
PACKED_BIAS = 256
PACKED_MAX_CELLS = 16383 - 2 * PACKED_BIAS


def unpack_selected(packed):
    """fpe_selected_packed records -> SELECTED_DTYPE records (foot_id / gait_cycle_id from the positions [..., n_cycles, 4])."""
    c = packed["cell"]
    out = np.zeros(packed.shape, dtype=SELECTED_DTYPE)
    out["row"] = (c & 0x3FFF).astype(np.int32) - PACKED_BIAS
    out["col"] = ((c >> 14) & 0x3FFF).astype(np.int32) - PACKED_BIAS
    out["z"] = packed["z"]
    out["valid"] = (c >> 28) & 1
    out["source"] = (c >> 29) & 3
    if packed.ndim >= 2:
        out["foot_id"] = np.arange(packed.shape[-1], dtype=np.uint8)
        out["gait_cycle_id"] = np.arange(packed.shape[-2], dtype=np.uint8)[:, None]
    return out


QUERY_DTYPE = np.dtype(
    [("cx", "<f8"), ("cy", "<f8"), ("search_radius", "<f4"), ("n_vertices", "<i4"),
     ("vx", "<f8", (MAX_POLYGON_VERTICES,)), ("vy", "<f8", (MAX_POLYGON_VERTICES,))],
    align=True,
)
MSG_FOOTHOLD_DTYPE = np.dtype(
    [("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("foot_id", "u1"), ("gait_cycle_id", "u1"), ("pad", "u1", (6,))],
    align=True,
)
GLOBAL_FOOTHOLDS_DTYPE = np.dtype(
    [("success", "u1"), ("gait_cycles", "u1"), ("gait_cycles_succeed", "u1"), ("pad", "u1"), ("n_footholds", "<i4"),
     ("footholds", MSG_FOOTHOLD_DTYPE, (4 + 4 * 255,))],
    align=True,
)


TRACK_REPORT_DTYPE = np.dtype(
    [("n_path", "<i4"), ("n_kpi", "<i4"), ("feet_center_path", "<f8", (510, 3)), ("feet_distance", "<f8", (510,)),
     ("cog_speed", "<f8", (510,))],
    align=True,
)
# the opt track (include/fpe.h: fpe_opt_params, fpe_opt_foothold, fpe_opt_cycle)
OPT_PARAMS_DTYPE = np.dtype(
    [("w1", "<f8"), ("w2", "<f8"), ("w3", "<f8"), ("w4", "<f8"), ("wr", "<f8"), ("wc", "<f8"),
     ("use_inequality_constraints", "<i4"), ("reserved", "<i4"), ("ctol", "<f8"),
     ("hip_lower_scale", "<f8"), ("hip_upper_scale", "<f8"), ("skew_lower_scale", "<f8"), ("skew_upper_scale", "<f8"),
     ("lf_current_row0", "<f8"), ("rh_current_row0", "<f8")],
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
assert OPT_FOOTHOLD_DTYPE.itemsize == 32 and OPT_CYCLE_DTYPE.itemsize == 240 and OPT_PARAMS_DTYPE.itemsize == 112


class MapDesc(C.Structure):
    _fields_ = [
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("resolution", C.c_double),
        ("position", C.c_double * 2),
        ("start_index", C.c_int32 * 2),
        ("storage_order", C.c_int32),
    ]


class PlanOut(C.Structure):
    _fields_ = [
        ("nominal", C.c_void_p),
        ("centroid", C.c_void_p),
        ("default_next", C.c_void_p),
        ("cycle_ok", C.c_void_p),
        ("stance", C.c_void_p),
        ("selected", C.c_void_p),
        ("pose_status", C.c_void_p),
        ("selected_packed", C.c_void_p),
    ]


class MultiDeviceIO(C.Structure):
    """fpe_multi_device_io: one device's block of a device-resident multi-GPU plan."""
    _fields_ = [("d_poses", C.c_void_p), ("d_out", PlanOut), ("d_gathered", C.c_void_p), ("stream", C.c_void_p)]


class ServiceGate(C.Structure):
    """fpe_service_gate: verdict of the handler's gate for the last service call of this thread."""
    _fields_ = [("fail_cycle", C.c_uint8), ("fail_kind", C.c_uint8), ("chain_ran", C.c_uint8), ("returned_false", C.c_uint8),
                ("pad", C.c_uint8 * 4), ("lf_current_row", C.c_double), ("rh_current_row", C.c_double)]


GATE_NONE, GATE_CYCLE0, GATE_LATERAL, GATE_BUILD_DEFINED = 0, 1, 2, 3
EXCHANGE_NONE, EXCHANGE_SELECTED, EXCHANGE_PACKED = 0, 1, 2


class OptOut(C.Structure):
    _fields_ = [("footholds", C.c_void_p), ("cycles", C.c_void_p), ("gate_fail_cycle", C.c_void_p), ("rows_after", C.c_void_p)]


class FilterParams(C.Structure):
    """fpe_filter_params (include/fpe.h): the producer's default filter chain."""
    _fields_ = [
        ("normal_radius", C.c_double),
        ("slope_critical", C.c_double),
        ("step_critical", C.c_double),
        ("step_first_radius", C.c_double),
        ("step_second_radius", C.c_double),
        ("step_critical_cells", C.c_int32),
        ("reserved", C.c_int32),
        ("roughness_critical", C.c_double),
        ("roughness_radius", C.c_double),
    ]


FMAP_DEFAULT_OK, FMAP_CANDIDATE_OK, FMAP_UNKNOWN = 1, 2, 4  # FPE_FMAP_* bits of fpe_foothold_map_out.flags


class FootholdMapOut(C.Structure):
    """fpe_foothold_map_out: products of a dense foothold-map call (either pointer may be NULL)."""
    _fields_ = [("flags", C.c_void_p), ("height", C.c_void_p)]


class FootholdSnapOut(C.Structure):
    """fpe_foothold_snap_out: products of a dense snap-map call (any pointer may be NULL)."""
    _fields_ = [("offset", C.c_void_p), ("source", C.c_void_p), ("z", C.c_void_p)]


class CentroidQuery(C.Structure):
    """fpe_centroid_query: the foothold the centroid method starts from and its search radius (<= 0: params.searchRadius)."""
    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("search_radius", C.c_float), ("pad", C.c_int32)]


CENTROID_QUERY_DTYPE = np.dtype(CentroidQuery)  # the array form of the same 24 bytes


class CentroidMapOut(C.Structure):
    """fpe_centroid_map_out: products of a dense centroid-map call (any pointer may be NULL)."""
    _fields_ = [("code", C.c_void_p), ("offset", C.c_void_p), ("z", C.c_void_p)]


# FPE_LAYER_* ids of include/fpe.h by name, in id order: the message layers fpe_export_layers* writes
LAYER_NAMES = ("foothold_flags", "foothold_height", "snap_di", "snap_dj", "snap_source", "snap_z", "centroid_code", "centroid_di",
               "centroid_dj", "centroid_z")
LAYER_COUNT = len(LAYER_NAMES)


class LayerLayout(C.Structure):
    """fpe_layer_layout: start index and storage order (0 column-major, 1 row-major) of the destination buffers."""
    _fields_ = [("start_index", C.c_int32 * 2), ("storage_order", C.c_int32), ("reserved", C.c_int32)]


class LayerRequest(C.Structure):
    """fpe_layer_request: the layers of one fpe_export_layers* call and where each goes (rows * cols floats of the whole map)."""
    _fields_ = [("n_layers", C.c_int32), ("layer", C.c_int32 * LAYER_COUNT), ("dst", C.c_void_p * LAYER_COUNT),
                ("snap_search_radius", C.c_float), ("snap_polygon_kind", C.c_int32), ("centroid_search_radius", C.c_float),
                ("reserved", C.c_int32)]


class PoseSummary(C.Structure):
    """fpe_pose_summary: what fpe_plan_rank* reduces one pose's plan to (64 bytes)."""
    _fields_ = [("success", C.c_uint8), ("gait_cycles_succeed", C.c_uint8), ("committed", C.c_uint8), ("first_failed", C.c_uint8),
                ("pose_status", C.c_uint8), ("pad", C.c_uint8 * 3), ("n_source", C.c_uint16 * 4), ("cog_speed_sum", C.c_double),
                ("cog_speed_min", C.c_double), ("cog_speed_max", C.c_double), ("feet_distance_min", C.c_double),
                ("feet_distance_max", C.c_double), ("deviation_sq_sum", C.c_double)]


class RankParams(C.Structure):
    """fpe_rank_params: the score's weights and the class-1 threshold."""
    _fields_ = [("w_fail", C.c_double), ("w_spiral", C.c_double), ("w_none", C.c_double), ("w_deviation", C.c_double),
                ("w_speed_spread", C.c_double), ("min_cycles", C.c_int32), ("reserved", C.c_int32)]


POSE_SUMMARY_DTYPE, RANK_PARAMS_DTYPE = np.dtype(PoseSummary), np.dtype(RankParams)  # the array forms


class RankOut(C.Structure):
    """fpe_rank_out: outputs of a ranking call (`best` is required; anything else may be NULL)."""
    _fields_ = [("summary", C.c_void_p), ("score", C.c_void_p), ("best", C.c_void_p), ("n_class0", C.c_void_p),
                ("best_products", PlanOut)]


BEAM_MAX_OPTIONS, BEAM_MAX_WIDTH, BEAM_MAX_CHAINS = 16, 64, 1 << 20  # FPE_BEAM_MAX_*


class BeamParams(C.Structure):
    """fpe_beam_params: the shape of a beam search over stride options (segments x cycles, entries kept per root) and its weights."""
    _fields_ = [("segments", C.c_int32), ("cycles_per_segment", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32),
                ("w_fail", C.c_double), ("w_spiral", C.c_double), ("w_none", C.c_double), ("w_deviation", C.c_double),
                ("w_progress", C.c_double)]


class BeamOut(C.Structure):
    """fpe_beam_out: outputs of a beam call (`path` is required; anything else may be NULL; no stance, no pose_status)."""
    _fields_ = [("n_live", C.c_void_p), ("score", C.c_void_p), ("penalty", C.c_void_p), ("path", C.c_void_p), ("state", C.c_void_p),
                ("products", PlanOut)]


UPDATE_MAX_PATCHES = 8  # FPE_UPDATE_MAX_PATCHES


class MapPatch(C.Structure):
    """fpe_map_patch: a rectangle of the NEW map and where its two layers lie (element (r, c) at r * row_stride + c * col_stride floats)."""
    _fields_ = [("row0", C.c_int32), ("col0", C.c_int32), ("n_rows", C.c_int32), ("n_cols", C.c_int32), ("traversability", C.c_void_p),
                ("elevation", C.c_void_p), ("row_stride", C.c_int64), ("col_stride", C.c_int64)]


class MapUpdate(C.Structure):
    """fpe_map_update: the current snapshot shifted by whole cells, with up to UPDATE_MAX_PATCHES rectangles replaced."""
    _fields_ = [("shift", C.c_int32 * 2), ("position", C.c_double * 2), ("n_patches", C.c_int32), ("reserved", C.c_int32),
                ("patch", MapPatch * UPDATE_MAX_PATCHES)]


class ElevationUpdateInfo(C.Structure):
    """fpe_elevation_update_info: what an elevation-driven update recomputed (reach R, route, |D|, cells the chain stored)."""
    _fields_ = [("reach_cells", C.c_int32), ("route", C.c_int32), ("dirty_cells", C.c_int64), ("recomputed_cells", C.c_int64)]


# FPE_SWING_* flag bits of fpe_swing_record.flags and the radius bound of a swing segment
SWING_SEGMENT, SWING_OFF_MAP, SWING_EMPTY, SWING_UNKNOWN, SWING_OVER_LIFT, SWING_OVER_RISE, SWING_OVER_LENGTH, SWING_REFUSED = (
    1, 2, 4, 8, 16, 32, 64, 128)
SWING_MAX_RADIUS = np.float32(0.5)
# fpe_swing_query: one segment A -> B with its capsule radius (<= 0: the limits' radius, else params.footRadius)
SWING_QUERY_DTYPE = np.dtype([("a", "<f8", (3,)), ("b", "<f8", (3,)), ("radius", "<f4"), ("reserved", "<i4")], align=True)
# fpe_swing_record: what a segment's capsule holds of the elevation layer; fpe_swing_summary: one pose's records reduced
SWING_RECORD_DTYPE = np.dtype(
    [("lift", "<f8"), ("rise", "<f8"), ("length_sq", "<f8"), ("max_elevation", "<f4"), ("n_cells", "<i4"), ("n_unknown", "<i4"),
     ("row", "<i4"), ("col", "<i4"), ("flags", "u1"), ("foot_id", "u1"), ("gait_cycle_id", "u1"), ("pad", "u1")],
    align=True,
)
SWING_SUMMARY_DTYPE = np.dtype(
    [("max_lift", "<f8"), ("max_abs_rise", "<f8"), ("max_length_sq", "<f8"), ("n_segments", "<i4"), ("n_over", "<i4"),
     ("n_unknown", "<i4"), ("first_over_cycle", "u1"), ("pad", "u1", (3,))],
    align=True,
)
assert (SWING_QUERY_DTYPE.itemsize, SWING_RECORD_DTYPE.itemsize, SWING_SUMMARY_DTYPE.itemsize) == (56, 48, 40)


class SwingLimits(C.Structure):
    """fpe_swing_limits: the three limits behind the OVER bits (+infinity: none) and the default capsule radius."""
    _fields_ = [("max_lift", C.c_double), ("max_rise", C.c_double), ("max_length", C.c_double), ("radius", C.c_float),
                ("reserved", C.c_int32)]


class SwingOut(C.Structure):
    """fpe_swing_out: outputs of a plan-bound swing check (either pointer may be NULL)."""
    _fields_ = [("records", C.c_void_p), ("summary", C.c_void_p)]


# FPE_TRUNK_* flag bits of fpe_trunk_record.flags and the bounds of a trunk stance
TRUNK_STANCE, TRUNK_OFF_MAP, TRUNK_EMPTY, TRUNK_UNKNOWN, TRUNK_UNDER_CLEARANCE, TRUNK_OVER_SLOPE, TRUNK_DEGENERATE, TRUNK_REFUSED = (
    1, 2, 4, 8, 16, 32, 64, 128)
TRUNK_MAX_HALF_EXTENT = np.float32(1.0)
TRUNK_MAX_CELLS = 65536
TRUNK_MAX_SLOPE = 1e6
# fpe_trunk_query: one stance, the feet RF, RH, LH, LF (x, y, z) and the box's half extents (<= 0: the limits', else half the params')
TRUNK_QUERY_DTYPE = np.dtype([("feet", "<f8", (4, 3)), ("half_length", "<f4"), ("half_width", "<f4"), ("reserved", "<i4", (2,))], align=True)
# fpe_trunk_record: what a stance's body box holds of the elevation layer; fpe_trunk_summary: one pose's records reduced
TRUNK_RECORD_DTYPE = np.dtype(
    [("clearance", "<f8"), ("slope_x", "<f8"), ("slope_y", "<f8"), ("base_z", "<f8"), ("max_elevation", "<f4"), ("n_cells", "<i4"),
     ("n_unknown", "<i4"), ("row", "<i4"), ("col", "<i4"), ("flags", "u1"), ("gait_cycle_id", "u1"), ("pad", "u1", (2,))],
    align=True,
)
TRUNK_SUMMARY_DTYPE = np.dtype(
    [("min_clearance", "<f8"), ("max_abs_slope_x", "<f8"), ("max_abs_slope_y", "<f8"), ("n_stances", "<i4"), ("n_bad", "<i4"),
     ("n_unknown", "<i4"), ("first_bad_cycle", "u1"), ("pad", "u1", (3,))],
    align=True,
)
assert (TRUNK_QUERY_DTYPE.itemsize, TRUNK_RECORD_DTYPE.itemsize, TRUNK_SUMMARY_DTYPE.itemsize) == (112, 56, 40)


class TrunkLimits(C.Structure):
    """fpe_trunk_limits: the limits behind UNDER_CLEARANCE / OVER_SLOPE (-/+infinity: none), the ride height and the default box."""
    _fields_ = [("min_clearance", C.c_double), ("max_slope_x", C.c_double), ("max_slope_y", C.c_double), ("ride_height", C.c_double),
                ("half_length", C.c_float), ("half_width", C.c_float), ("reserved", C.c_int32 * 2)]


class TrunkOut(C.Structure):
    """fpe_trunk_out: outputs of a plan-bound trunk check (either pointer may be NULL)."""
    _fields_ = [("records", C.c_void_p), ("summary", C.c_void_p)]


# FPE_MARGIN_* class bits of fpe_margin_params.classes, flag bits of fpe_margin_record.flags, and the bounds of a margin call
MARGIN_LOW_CANDIDATE, MARGIN_LOW_DEFAULT, MARGIN_UNKNOWN, MARGIN_OFF_MAP = 1, 2, 4, 8
MARGIN_FOOTHOLD, MARGIN_CENTRE_OFF_MAP, MARGIN_NO_BAD, MARGIN_UNDER, MARGIN_REFUSED = 1, 2, 4, 8, 128
MARGIN_MAX_CELLS = 31
MARGIN_NONE = 65535
# fpe_margin_query: one cell; fpe_margin_record: its margin; fpe_margin_summary: one pose's records reduced
MARGIN_QUERY_DTYPE = np.dtype([("row", "<i4"), ("col", "<i4")], align=True)
MARGIN_RECORD_DTYPE = np.dtype(
    [("dist_sq", "<u2"), ("di", "i1"), ("dj", "i1"), ("flags", "u1"), ("foot_id", "u1"), ("gait_cycle_id", "u1"), ("pad", "u1")], align=True)
MARGIN_SUMMARY_DTYPE = np.dtype(
    [("min_dist_sq", "<u2"), ("min_cycle", "u1"), ("min_leg", "u1"), ("n_footholds", "<u2"), ("n_under", "<u2"), ("n_off_map", "<u2"),
     ("first_under_cycle", "u1"), ("pad", "u1", (5,))],
    align=True,
)
assert (MARGIN_QUERY_DTYPE.itemsize, MARGIN_RECORD_DTYPE.itemsize, MARGIN_SUMMARY_DTYPE.itemsize) == (8, 8, 16)


class MarginParams(C.Structure):
    """fpe_margin_params: the class bits that make a cell BAD, the reach in cells and the limit behind UNDER (0: none)."""
    _fields_ = [("classes", C.c_int32), ("reach_cells", C.c_int32), ("min_margin", C.c_double), ("reserved", C.c_int32 * 2)]


class MarginMapOut(C.Structure):
    """fpe_margin_map_out: products of a dense margin call (either pointer may be NULL, not both)."""
    _fields_ = [("dist_sq", C.c_void_p), ("nearest", C.c_void_p)]


class MarginOut(C.Structure):
    """fpe_margin_out: outputs of a plan-bound margin call (either pointer may be NULL, not both)."""
    _fields_ = [("records", C.c_void_p), ("summary", C.c_void_p)]


CHECK_SWING, CHECK_TRUNK, CHECK_MARGIN, CHECK_UNKNOWN = 1, 2, 4, 8  # FPE_CHECK_* bits of fpe_check_params and of fpe_check_out.hit


class CheckParams(C.Structure):
    """fpe_check_params: the checks a checked ranking folds into its score (FPE_CHECK_* bits), the hit bits that move a pose to class
    1, the weights of the score's check terms and the three checks' own limit blocks (read only when their check is enabled)."""
    _fields_ = [("checks", C.c_uint32), ("reject", C.c_uint32), ("w_swing_over", C.c_double), ("w_lift", C.c_double),
                ("w_trunk_bad", C.c_double), ("w_margin_under", C.c_double), ("w_unknown", C.c_double), ("reserved", C.c_double),
                ("swing", SwingLimits), ("trunk", TrunkLimits), ("margin", MarginParams)]


class CheckOut(C.Structure):
    """fpe_check_out: the check outputs of a checked ranking, one element per pose (any pointer may be NULL)."""
    _fields_ = [("swing", C.c_void_p), ("trunk", C.c_void_p), ("margin", C.c_void_p), ("base_score", C.c_void_p), ("hit", C.c_void_p)]


class BeamCheckOut(C.Structure):
    """fpe_beam_check_out: the check outputs of a checked beam, one element per slot (b, w) (any pointer may be NULL)."""
    _fields_ = [("swing", C.c_void_p), ("trunk", C.c_void_p), ("margin", C.c_void_p), ("base_penalty", C.c_void_p), ("hit", C.c_void_p),
                ("feet", C.c_void_p)]


assert (C.sizeof(CheckParams), C.sizeof(CheckOut), C.sizeof(BeamCheckOut)) == (160, 40, 48)

SCAN_MAX_POINTS = 1 << 22  # FPE_SCAN_MAX_POINTS


class ScanParams(C.Structure):
    """fpe_scan_params: the point tests (range, height window), the surface band, the variance model and the gate of a scan fusion."""
    _fields_ = [("min_range", C.c_float), ("max_range", C.c_float), ("min_z", C.c_float), ("max_z", C.c_float), ("band", C.c_float),
                ("var_base", C.c_float), ("var_range", C.c_float), ("var_min", C.c_float), ("var_max", C.c_float), ("gate", C.c_float),
                ("var_outlier", C.c_float), ("replace_count", C.c_int32)]


class Scan(C.Structure):
    """fpe_scan: one scan's sensor-to-map transform (row-major 3 x 4), point count and stride, and the roi it may write."""
    _fields_ = [("sensor_to_map", C.c_double * 12), ("n_points", C.c_int32), ("point_stride", C.c_int32), ("roi", C.c_int32 * 4),
                ("reserved", C.c_int32 * 2)]


# fpe_scan_info: sixteen int32 (the array form is what a device info is read back as)
SCAN_INFO_DTYPE = np.dtype(
    [("n_points", "<i4"), ("dropped_nonfinite", "<i4"), ("dropped_range", "<i4"), ("dropped_height", "<i4"), ("dropped_off_roi", "<i4"),
     ("accepted", "<i4"), ("below_band", "<i4"), ("cells_touched", "<i4"), ("cells_new", "<i4"), ("cells_fused", "<i4"),
     ("cells_outlier", "<i4"), ("cells_replaced", "<i4"), ("bbox", "<i4", (4,))],
    align=True,
)
assert (C.sizeof(ScanParams), C.sizeof(Scan), SCAN_INFO_DTYPE.itemsize) == (48, 128, 64)


class ScanClearParams(C.Structure):
    """fpe_scan_clear_params: how the rays of a visibility clearing are sampled and when a cell they pass below becomes unknown."""
    _fields_ = [("sample_step", C.c_float), ("margin", C.c_float), ("start_samples", C.c_int32), ("end_samples", C.c_int32),
                ("min_hits", C.c_int32), ("ray_stride", C.c_int32), ("max_samples", C.c_int32), ("reserved", C.c_int32)]


# fpe_scan_clear_info: twelve int32 and two int64 (sixteen int32 words when a device info is read back)
SCAN_CLEAR_INFO_DTYPE = np.dtype(
    [("n_points", "<i4"), ("strided_out", "<i4"), ("dropped_points", "<i4"), ("rays", "<i4"), ("rays_long", "<i4"), ("rays_empty", "<i4"),
     ("cells_hit", "<i4"), ("cells_cleared", "<i4"), ("bbox", "<i4", (4,)), ("samples_in_roi", "<i8"), ("hit_pairs", "<i8")],
    align=True,
)
assert (C.sizeof(ScanClearParams), SCAN_CLEAR_INFO_DTYPE.itemsize) == (32, 64)


class ScanCloseParams(C.Structure):
    """fpe_scan_close_params: how far a gap closing searches, how wide a gap it bridges, how many axes must span a cell and how far
    their end heights may lie apart."""
    _fields_ = [("reach", C.c_int32), ("max_gap", C.c_int32), ("min_axes", C.c_int32), ("max_spread", C.c_float), ("reserved", C.c_int32 * 4)]


# fpe_scan_close_info: sixteen int32
SCAN_CLOSE_INFO_DTYPE = np.dtype(
    [("cells", "<i4"), ("known", "<i4"), ("unknown", "<i4"), ("filled", "<i4"), ("no_support", "<i4"), ("rejected_axes", "<i4"),
     ("rejected_spread", "<i4"), ("reserved", "<i4"), ("bbox", "<i4", (4,)), ("reserved2", "<i4", (4,))],
    align=True,
)
assert (C.sizeof(ScanCloseParams), SCAN_CLOSE_INFO_DTYPE.itemsize) == (32, 64)

SCAN_IMAGE_PINHOLE, SCAN_IMAGE_SPHERICAL = 0, 1  # FPE_SCAN_IMAGE_*
SCAN_DEPTH_U16, SCAN_DEPTH_F32 = 0, 1            # FPE_SCAN_DEPTH_*


class ScanImage(C.Structure):
    """fpe_scan_image: how the pixels of a depth or range image become points (model, format, size, pitch, steps, scale, the pinhole
    intrinsics or the two direction tables)."""
    _fields_ = [("model", C.c_int32), ("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("row_pitch", C.c_int32),
                ("row_step", C.c_int32), ("col_step", C.c_int32), ("depth_scale", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("reserved", C.c_int32 * 2), ("row_dir", C.c_void_p), ("col_dir", C.c_void_p)]


assert C.sizeof(ScanImage) == 72

ABI_VERSION = 5  # FPE_ABI_VERSION of include/fpe.h: the layout the mirrors above have
# every struct of include/fpe.h -> its mirror (tests/test_cpu_abi.py checks each against the C compiler, and the key set against the header)
STRUCTS = {
    "fpe_params": PARAMS_DTYPE, "fpe_pose": POSE_DTYPE, "fpe_map_desc": MapDesc, "fpe_foothold": FOOTHOLD_DTYPE,
    "fpe_centroid_foothold": CENTROID_DTYPE, "fpe_selected_foothold": SELECTED_DTYPE, "fpe_selected_packed": PACKED_DTYPE,
    "fpe_plan_out": PlanOut, "fpe_opt_params": OPT_PARAMS_DTYPE, "fpe_opt_foothold": OPT_FOOTHOLD_DTYPE,
    "fpe_opt_cycle": OPT_CYCLE_DTYPE, "fpe_opt_out": OptOut, "fpe_leg_query": QUERY_DTYPE, "fpe_msg_foothold": MSG_FOOTHOLD_DTYPE,
    "fpe_global_footholds": GLOBAL_FOOTHOLDS_DTYPE, "fpe_filter_params": FilterParams, "fpe_service_gate": ServiceGate,
    "fpe_track_report": TRACK_REPORT_DTYPE, "fpe_multi_device_io": MultiDeviceIO, "fpe_foothold_map_out": FootholdMapOut,
    "fpe_foothold_snap_out": FootholdSnapOut, "fpe_centroid_query": CentroidQuery, "fpe_centroid_map_out": CentroidMapOut,
    "fpe_pose_summary": PoseSummary, "fpe_rank_params": RankParams, "fpe_rank_out": RankOut, "fpe_layer_layout": LayerLayout,
    "fpe_layer_request": LayerRequest, "fpe_stride": STRIDE_DTYPE, "fpe_plan_state": PLAN_STATE_DTYPE,
    "fpe_beam_params": BeamParams, "fpe_beam_out": BeamOut, "fpe_map_patch": MapPatch, "fpe_map_update": MapUpdate,
    "fpe_elevation_update_info": ElevationUpdateInfo, "fpe_swing_query": SWING_QUERY_DTYPE, "fpe_swing_limits": SwingLimits,
    "fpe_swing_record": SWING_RECORD_DTYPE, "fpe_swing_summary": SWING_SUMMARY_DTYPE, "fpe_swing_out": SwingOut,
    "fpe_trunk_query": TRUNK_QUERY_DTYPE, "fpe_trunk_limits": TrunkLimits, "fpe_trunk_record": TRUNK_RECORD_DTYPE,
    "fpe_trunk_summary": TRUNK_SUMMARY_DTYPE, "fpe_trunk_out": TrunkOut,
    "fpe_margin_params": MarginParams, "fpe_margin_map_out": MarginMapOut, "fpe_margin_query": MARGIN_QUERY_DTYPE,
    "fpe_margin_record": MARGIN_RECORD_DTYPE, "fpe_margin_summary": MARGIN_SUMMARY_DTYPE, "fpe_margin_out": MarginOut,
    "fpe_check_params": CheckParams, "fpe_check_out": CheckOut, "fpe_beam_check_out": BeamCheckOut,
    "fpe_scan_params": ScanParams, "fpe_scan": Scan, "fpe_scan_info": SCAN_INFO_DTYPE,
    "fpe_scan_clear_params": ScanClearParams, "fpe_scan_clear_info": SCAN_CLEAR_INFO_DTYPE,
    "fpe_scan_close_params": ScanCloseParams, "fpe_scan_close_info": SCAN_CLOSE_INFO_DTYPE, "fpe_scan_image": ScanImage,
}
FILTER_LAYERS = ("normal_x", "normal_y", "normal_z", "slope", "step_height", "step", "roughness", "traversability")

# every entry point include/fpe.h declares -> (restype, argtypes); lib() applies the table, tests check it names exactly the
# header's functions and that the library exports each of them
vp, cint, i32, u8, f32, f64, cstr, P = C.c_void_p, C.c_int, C.c_int32, C.c_uint8, C.c_float, C.c_double, C.c_char_p, C.POINTER
PROTOTYPES = {
    "fpe_params_yaml": (cint, [vp]),
    "fpe_params_code_defaults": (cint, [vp]),
    "fpe_create": (cint, [cint, P(vp)]),
    "fpe_destroy": (cint, [vp]),
    "fpe_last_error": (cstr, [vp]),
    "fpe_version": (cstr, []),
    "fpe_abi_version": (cint, []),
    "fpe_upload_map": (cint, [vp, P(MapDesc), vp, vp]),
    "fpe_upload_map_device": (cint, [vp, P(MapDesc), vp, vp, vp]),
    "fpe_map_info": (cint, [vp, P(MapDesc)]),
    "fpe_update_map": (cint, [vp, P(MapUpdate)]),
    "fpe_update_map_device": (cint, [vp, P(MapUpdate), vp]),
    "fpe_map_update_validate": (cint, [P(MapDesc), P(MapUpdate)]),
    "fpe_filter_reach_cells": (cint, [P(FilterParams), f64]),
    "fpe_elevation_update_plan": (cint, [P(MapDesc), P(FilterParams), P(MapUpdate), P(ElevationUpdateInfo), vp]),
    "fpe_update_elevation": (cint, [vp, P(FilterParams), P(MapUpdate), P(ElevationUpdateInfo)]),
    "fpe_update_elevation_device": (cint, [vp, P(FilterParams), P(MapUpdate), P(ElevationUpdateInfo), vp]),
    "fpe_read_map_layers": (cint, [vp, vp, vp]),
    "fpe_read_map_layers_device": (cint, [vp, vp, vp, vp]),
    "fpe_filter_params_defaults": (cint, [P(FilterParams)]),
    "fpe_traversability": (cint, [vp, P(MapDesc), P(FilterParams), vp, vp, vp]),
    "fpe_traversability_device": (cint, [vp, P(MapDesc), P(FilterParams), vp, vp, vp, vp]),
    "fpe_set_max_leg_search_radius": (cint, [vp, f32]),
    "fpe_set_tuning": (cint, [vp, cstr, i32]),
    "fpe_describe_plan": (cint, [vp, vp, cstr, i32]),
    "fpe_host_alloc": (cint, [vp, C.c_size_t, P(vp)]),
    "fpe_host_free": (cint, [vp, vp]),
    "fpe_plan": (cint, [vp, vp, vp, i32, i32, P(PlanOut)]),
    "fpe_plan_device": (cint, [vp, vp, vp, i32, i32, P(PlanOut), vp]),
    "fpe_search_legs": (cint, [vp, vp, vp, i32, vp]),
    "fpe_search_legs_device": (cint, [vp, vp, vp, i32, vp, vp]),
    "fpe_plan_service": (cint, [vp, vp, vp, u8, vp]),
    "fpe_plan_service_ex": (cint, [vp, vp, vp, u8, vp, vp, vp, vp]),
    "fpe_plan_service_report": (cint, [vp, vp, vp, u8, vp, vp, vp, vp, vp, vp]),
    "fpe_plan_service_opt": (cint, [vp, vp, vp, vp, u8] + [vp] * 9),
    "fpe_last_service_gate": (cint, [vp, P(ServiceGate)]),
    "fpe_opt_params_yaml": (cint, [vp]),
    "fpe_opt_params_code_defaults": (cint, [vp]),
    "fpe_plan_opt": (cint, [vp, vp, vp, vp, i32, i32, vp, P(OptOut)]),
    "fpe_plan_opt_device": (cint, [vp, vp, vp, vp, i32, i32, vp, P(OptOut), vp]),
    "fpe_multi_create": (cint, [vp, i32, P(vp)]),
    "fpe_multi_destroy": (cint, [vp]),
    "fpe_multi_device_count": (cint, [vp]),
    "fpe_multi_engine": (vp, [vp, i32]),
    "fpe_multi_last_error": (cstr, [vp]),
    "fpe_multi_upload_map": (cint, [vp, P(MapDesc), vp, vp]),
    "fpe_multi_update_map": (cint, [vp, P(MapUpdate)]),
    "fpe_multi_set_tuning": (cint, [vp, cstr, i32]),
    "fpe_multi_plan": (cint, [vp, vp, vp, i32, i32, P(PlanOut)]),
    "fpe_multi_shard_range": (cint, [i32, i32, i32, P(i32), P(i32)]),
    "fpe_multi_plan_device": (cint, [vp, vp, P(MultiDeviceIO), i32, i32, i32]),
    "fpe_multi_stream": (vp, [vp, i32]),
    "fpe_multi_synchronize": (cint, [vp]),
    "fpe_foothold_map": (cint, [vp, vp, vp, P(FootholdMapOut)]),
    "fpe_foothold_map_device": (cint, [vp, vp, vp, P(FootholdMapOut), vp]),
    "fpe_foothold_snap": (cint, [vp, vp, vp, f32, i32, P(FootholdSnapOut)]),
    "fpe_foothold_snap_device": (cint, [vp, vp, vp, f32, i32, P(FootholdSnapOut), vp]),
    "fpe_centroid_legs": (cint, [vp, vp, vp, i32, vp]),
    "fpe_centroid_legs_device": (cint, [vp, vp, vp, i32, vp, vp]),
    "fpe_centroid_map": (cint, [vp, vp, vp, f32, P(CentroidMapOut)]),
    "fpe_centroid_map_device": (cint, [vp, vp, vp, f32, P(CentroidMapOut), vp]),
    "fpe_rank_params_defaults": (cint, [P(RankParams)]),
    "fpe_plan_rank": (cint, [vp, vp, P(RankParams), vp, i32, i32, i32, P(RankOut)]),
    "fpe_plan_rank_device": (cint, [vp, vp, P(RankParams), vp, i32, i32, i32, P(PlanOut), P(RankOut), vp]),
    "fpe_export_layers": (cint, [vp, vp, vp, P(LayerLayout), P(LayerRequest)]),
    "fpe_export_layers_device": (cint, [vp, vp, vp, P(LayerLayout), P(LayerRequest), vp]),
    "fpe_plan_strides": (cint, [vp, vp, vp, vp, i32, i32, P(PlanOut)]),
    "fpe_plan_strides_device": (cint, [vp, vp, vp, vp, i32, i32, P(PlanOut), vp]),
    "fpe_plan_rank_strides": (cint, [vp, vp, P(RankParams), vp, vp, i32, i32, i32, P(RankOut)]),
    "fpe_plan_rank_strides_device": (cint, [vp, vp, P(RankParams), vp, vp, i32, i32, i32, P(PlanOut), P(RankOut), vp]),
    "fpe_describe_plan_strides": (cint, [vp, vp, cstr, i32]),
    "fpe_plan_resume": (cint, [vp, vp, vp, vp, vp, i32, i32, P(PlanOut), vp]),
    "fpe_plan_resume_device": (cint, [vp, vp, vp, vp, vp, i32, i32, P(PlanOut), vp, vp]),
    "fpe_plan_state_from_pose": (cint, [vp, vp, vp, vp]),
    "fpe_plan_state_from_feet": (cint, [vp, f64, i32, vp]),
    "fpe_describe_plan_resume": (cint, [vp, vp, cstr, i32]),
    "fpe_beam_params_defaults": (cint, [P(BeamParams)]),
    "fpe_plan_beam": (cint, [vp, vp, P(BeamParams), vp, vp, i32, vp, i32, P(BeamOut)]),
    "fpe_plan_beam_device": (cint, [vp, vp, P(BeamParams), vp, vp, i32, vp, i32, P(BeamOut), vp]),
    "fpe_swing_limits_defaults": (cint, [P(SwingLimits)]),
    "fpe_swing_segments": (cint, [vp, vp, P(SwingLimits), vp, i32, vp]),
    "fpe_swing_segments_device": (cint, [vp, vp, P(SwingLimits), vp, i32, vp, vp]),
    "fpe_swing_plan_device": (cint, [vp, vp, P(SwingLimits), P(PlanOut), vp, i32, i32, P(SwingOut), vp]),
    "fpe_swing_plan": (cint, [vp, vp, P(SwingLimits), vp, vp, i32, i32, P(PlanOut), P(SwingOut)]),
    "fpe_trunk_limits_defaults": (cint, [P(TrunkLimits)]),
    "fpe_trunk_stances": (cint, [vp, vp, P(TrunkLimits), vp, i32, vp]),
    "fpe_trunk_stances_device": (cint, [vp, vp, P(TrunkLimits), vp, i32, vp, vp]),
    "fpe_trunk_plan_device": (cint, [vp, vp, P(TrunkLimits), P(PlanOut), i32, i32, P(TrunkOut), vp]),
    "fpe_trunk_plan": (cint, [vp, vp, P(TrunkLimits), vp, vp, i32, i32, P(PlanOut), P(TrunkOut)]),
    "fpe_margin_params_defaults": (cint, [P(MarginParams)]),
    "fpe_margin_map": (cint, [vp, vp, P(MarginParams), vp, P(MarginMapOut)]),
    "fpe_margin_map_device": (cint, [vp, vp, P(MarginParams), vp, P(MarginMapOut), vp]),
    "fpe_margin_cells": (cint, [vp, vp, P(MarginParams), vp, i32, vp]),
    "fpe_margin_cells_device": (cint, [vp, vp, P(MarginParams), vp, i32, vp, vp]),
    "fpe_margin_plan_device": (cint, [vp, vp, P(MarginParams), P(PlanOut), i32, i32, P(MarginOut), vp]),
    "fpe_margin_plan": (cint, [vp, vp, P(MarginParams), vp, vp, i32, i32, P(PlanOut), P(MarginOut)]),
    "fpe_check_params_defaults": (cint, [P(CheckParams)]),
    "fpe_check_plan_device": (cint, [vp, vp, P(CheckParams), P(PlanOut), vp, i32, i32, P(CheckOut), vp]),
    "fpe_plan_rank_checked_device": (cint, [vp, vp, P(RankParams), P(CheckParams), vp, vp, i32, i32, i32, P(PlanOut), P(RankOut),
                                            P(CheckOut), vp]),
    "fpe_plan_rank_checked": (cint, [vp, vp, P(RankParams), P(CheckParams), vp, vp, i32, i32, i32, P(RankOut), P(CheckOut)]),
    "fpe_plan_beam_checked": (cint, [vp, vp, P(BeamParams), P(CheckParams), vp, vp, vp, i32, vp, i32, P(BeamOut), P(BeamCheckOut)]),
    "fpe_plan_beam_checked_device": (cint, [vp, vp, P(BeamParams), P(CheckParams), vp, vp, vp, i32, vp, i32, P(BeamOut), P(BeamCheckOut),
                                            vp]),
    "fpe_scan_params_defaults": (cint, [P(ScanParams)]),
    "fpe_scan_validate": (cint, [P(MapDesc), P(ScanParams), P(Scan)]),
    "fpe_scan_create": (cint, [vp, P(MapDesc), P(vp)]),
    "fpe_scan_destroy": (cint, [vp]),
    "fpe_scan_geometry": (cint, [vp, P(MapDesc)]),
    "fpe_scan_set_layers": (cint, [vp, vp, vp]),
    "fpe_scan_set_layers_device": (cint, [vp, vp, vp, vp]),
    "fpe_scan_read_layers": (cint, [vp, vp, vp]),
    "fpe_scan_read_layers_device": (cint, [vp, vp, vp, vp]),
    "fpe_scan_move": (cint, [vp, P(i32), P(f64), vp]),
    "fpe_scan_fuse": (cint, [vp, P(ScanParams), P(Scan), vp, vp]),
    "fpe_scan_fuse_device": (cint, [vp, P(ScanParams), P(Scan), vp, vp, vp]),
    "fpe_scan_install": (cint, [vp, vp, P(FilterParams), vp]),
    "fpe_scan_ingest": (cint, [vp, vp, P(FilterParams), P(ScanParams), P(Scan), vp, P(i32), P(f64), vp, P(ElevationUpdateInfo)]),
    "fpe_scan_ingest_device": (cint, [vp, vp, P(FilterParams), P(ScanParams), P(Scan), vp, P(i32), P(f64), vp, P(ElevationUpdateInfo), vp]),
    "fpe_scan_clear_params_defaults": (cint, [P(ScanClearParams)]),
    "fpe_scan_clear_validate": (cint, [P(MapDesc), P(ScanParams), P(ScanClearParams), P(Scan)]),
    "fpe_scan_clear": (cint, [vp, P(ScanParams), P(ScanClearParams), P(Scan), vp, vp]),
    "fpe_scan_clear_device": (cint, [vp, P(ScanParams), P(ScanClearParams), P(Scan), vp, vp, vp]),
    "fpe_scan_ingest_clear": (cint, [vp, vp, P(FilterParams), P(ScanParams), P(ScanClearParams), P(Scan), vp, P(i32), P(f64), vp, vp,
                                     P(ElevationUpdateInfo)]),
    "fpe_scan_ingest_clear_device": (cint, [vp, vp, P(FilterParams), P(ScanParams), P(ScanClearParams), P(Scan), vp, P(i32), P(f64), vp, vp,
                                            P(ElevationUpdateInfo), vp]),
    "fpe_scan_close_params_defaults": (cint, [P(ScanCloseParams)]),
    "fpe_scan_close_validate": (cint, [P(MapDesc), P(ScanCloseParams), P(i32)]),
    "fpe_scan_close": (cint, [vp, P(ScanCloseParams), P(i32), vp, C.c_int64, vp, vp]),
    "fpe_scan_close_device": (cint, [vp, P(ScanCloseParams), P(i32), vp, C.c_int64, vp, vp, vp]),
    "fpe_scan_install_closed": (cint, [vp, vp, P(FilterParams), P(ScanCloseParams), vp]),
    "fpe_scan_ingest_closed": (cint, [vp, vp, P(FilterParams), P(ScanParams), P(ScanClearParams), P(ScanCloseParams), P(Scan), vp, P(i32), P(f64),
                                      vp, vp, vp, P(ElevationUpdateInfo)]),
    "fpe_scan_ingest_closed_device": (cint, [vp, vp, P(FilterParams), P(ScanParams), P(ScanClearParams), P(ScanCloseParams), P(Scan), vp, P(i32),
                                             P(f64), vp, vp, vp, P(ElevationUpdateInfo), vp]),
    "fpe_scan_image_validate": (cint, [P(MapDesc), P(ScanParams), P(ScanClearParams), P(Scan), P(ScanImage)]),
    "fpe_scan_image_points": (cint, [P(ScanImage), vp, vp]),
    "fpe_scan_fuse_image": (cint, [vp, P(ScanParams), P(Scan), P(ScanImage), vp, vp]),
    "fpe_scan_fuse_image_device": (cint, [vp, P(ScanParams), P(Scan), P(ScanImage), vp, vp, vp]),
    "fpe_scan_clear_image": (cint, [vp, P(ScanParams), P(ScanClearParams), P(Scan), P(ScanImage), vp, vp]),
    "fpe_scan_clear_image_device": (cint, [vp, P(ScanParams), P(ScanClearParams), P(Scan), P(ScanImage), vp, vp, vp]),
    "fpe_scan_ingest_image": (cint, [vp, vp, P(FilterParams), P(ScanParams), P(ScanClearParams), P(ScanCloseParams), P(Scan), P(ScanImage), vp,
                                     P(i32), P(f64), vp, vp, vp, P(ElevationUpdateInfo)]),
    "fpe_scan_ingest_image_device": (cint, [vp, vp, P(FilterParams), P(ScanParams), P(ScanClearParams), P(ScanCloseParams), P(Scan), P(ScanImage),
                                            vp, P(i32), P(f64), vp, vp, vp, P(ElevationUpdateInfo), vp]),
    "fpe_spiral_offsets": (cint, [i32, vp, i32]),
    "fpe_tile_halfwidth": (cint, [f32, f32, f64]),
    "fpe_algorithmic_bytes_per_foothold": (f64, [f32, f32, f64]),
}
EXPORTED_SYMBOLS = list(PROTOTYPES)

_lib = None


class EngineUnavailable(RuntimeError):
    """libfpe.so is missing / not loadable, or no gfx950 device: the product has no CPU path."""


def lib():
    """Load libfpe.so (building it with hipcc first if the in-tree .so is missing or stale)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # FPE_LIB: load a specific prebuilt engine (kernel-variant A/B runs); default = in-tree libfpe.so
        path = os.environ.get("FPE_LIB") or _build.build_engine()
    except Exception as e:  # hipcc missing or compile error: fail loudly — never load a stale library instead
        raise EngineUnavailable(f"cannot build libfpe.so: {e}") from e
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise EngineUnavailable(f"cannot load {path}: {e}") from e
    # a library that predates a symbol of include/fpe.h (FPE_LIB pointing at an old scratch build) is "unavailable", not an
    # AttributeError out of ctypes that callers catching EngineUnavailable would not see
    missing = [name for name in EXPORTED_SYMBOLS if not hasattr(L, name)]
    if missing:
        raise EngineUnavailable(f"{path} predates include/fpe.h (ABI version {ABI_VERSION}): it does not export {', '.join(missing[:4])}"
                                + (" ..." if len(missing) > 4 else ""))
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    if L.fpe_abi_version() != ABI_VERSION:
        raise EngineUnavailable(f"libfpe.so has struct layout version {L.fpe_abi_version()}, this binding mirrors version {ABI_VERSION} of include/fpe.h")
    _lib = L
    return L


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def params_yaml():
    p = np.zeros(1, dtype=PARAMS_DTYPE)
    assert lib().fpe_params_yaml(ptr(p)) == FPE_OK
    return p


def params_code_defaults():
    p = np.zeros(1, dtype=PARAMS_DTYPE)
    assert lib().fpe_params_code_defaults(ptr(p)) == FPE_OK
    return p


def opt_params_yaml():
    p = np.zeros(1, dtype=OPT_PARAMS_DTYPE)
    assert lib().fpe_opt_params_yaml(ptr(p)) == FPE_OK
    return p


def opt_params_code_defaults():
    p = np.zeros(1, dtype=OPT_PARAMS_DTYPE)
    assert lib().fpe_opt_params_code_defaults(ptr(p)) == FPE_OK
    return p


def rank_params_defaults(**overrides):
    """fpe_rank_params_defaults, with any field replaced by a keyword."""
    rp = RankParams()
    assert lib().fpe_rank_params_defaults(C.byref(rp)) == FPE_OK
    for k, v in overrides.items():
        if k not in dict(RankParams._fields_):
            raise ValueError(f"unknown rank parameter {k!r}")
        setattr(rp, k, v)
    return rp


def beam_params_defaults(**overrides):
    """fpe_beam_params_defaults, with any field replaced by a keyword."""
    bp = BeamParams()
    assert lib().fpe_beam_params_defaults(C.byref(bp)) == FPE_OK
    for k, v in overrides.items():
        if k not in dict(BeamParams._fields_):
            raise ValueError(f"unknown beam parameter {k!r}")
        setattr(bp, k, v)
    return bp


def swing_limits_defaults(**overrides):
    """fpe_swing_limits_defaults, with any field replaced by a keyword."""
    sl = SwingLimits()
    assert lib().fpe_swing_limits_defaults(C.byref(sl)) == FPE_OK
    for k, v in overrides.items():
        if k not in dict(SwingLimits._fields_):
            raise ValueError(f"unknown swing limit {k!r}")
        setattr(sl, k, v)
    return sl


def trunk_limits_defaults(**overrides):
    """fpe_trunk_limits_defaults, with any field replaced by a keyword."""
    tl = TrunkLimits()
    assert lib().fpe_trunk_limits_defaults(C.byref(tl)) == FPE_OK
    for k, v in overrides.items():
        if k not in dict(TrunkLimits._fields_) or k == "reserved":
            raise ValueError(f"unknown trunk limit {k!r}")
        setattr(tl, k, v)
    return tl


def check_params_defaults():
    """fpe_check_params_defaults: all three checks, no reject bit, the documented weights, each check's own default limits."""
    cp = CheckParams()
    assert lib().fpe_check_params_defaults(C.byref(cp)) == FPE_OK
    return cp


def spiral_offsets(n_rings):
    n = lib().fpe_spiral_offsets(n_rings, None, 0)
    if n < 0:
        raise ValueError("n_rings out of range")
    out = np.zeros((n, 3), dtype=np.int32)
    lib().fpe_spiral_offsets(n_rings, ptr(out), n)
    return out


def algorithmic_bytes_per_foothold(search_radius, foot_radius, resolution):
    return float(lib().fpe_algorithmic_bytes_per_foothold(np.float32(search_radius), np.float32(foot_radius), float(resolution)))
