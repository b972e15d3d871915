"""Host-side mirror of the reference's interface for the hot path, over the C ABI (include/fpe.h).

`FootholdPlanner` keeps the reference's names for the seam it replaces
(/root/reference/foothold_planner/src/FootholdPlanner.cpp): `gridmapCallback` (cpp:504),
`globalFootholdPlan` (cpp:539), `checkFoothold` (cpp:2001).  The batch entry points `plan` /
`plan_device` are the build-defined batch axis.  There is no CPU path: if
libfpe.so cannot be loaded or no gfx950 GPU is present, construction raises EngineUnavailable.
"""
import contextlib
import ctypes as C

import threading

import numpy as np

from . import _capi
from ._capi import (CENTROID_DTYPE, CENTROID_QUERY_DTYPE, FOOTHOLD_DTYPE, GLOBAL_FOOTHOLDS_DTYPE, OPT_CYCLE_DTYPE, OPT_FOOTHOLD_DTYPE, OPT_PARAMS_DTYPE,
                    PACKED_DTYPE, PLAN_STATE_DTYPE, POSE_DTYPE, PARAMS_DTYPE, QUERY_DTYPE, SELECTED_DTYPE, STRIDE_DTYPE, TRACK_REPORT_DTYPE, EngineUnavailable,
                    CentroidMapOut, FootholdMapOut, FootholdSnapOut, MapDesc, OptOut, PlanOut, RankOut, ptr)

# products of a chained plan in the order of fpe_plan_out's fields (= the order of the engine's device arena)
PRODUCT_ORDER = ("nominal", "centroid", "default", "cycle_ok", "stance", "selected", "pose_status", "selected_packed")
PRODUCT_FIELDS = dict(zip(PRODUCT_ORDER, (name for name, _ in PlanOut._fields_)))  # ("default" is fpe_plan_out.default_next)
DEFAULT_PRODUCTS = PRODUCT_ORDER[:7]  # what a plan returns when `products` is left out: everything but the 8-byte exchange record


def product_shapes(B, n_cycles):
    return {
        "nominal": ((B, n_cycles, 4), FOOTHOLD_DTYPE), "centroid": ((B, n_cycles, 4), CENTROID_DTYPE),
        "default": ((B, n_cycles, 4, 3), np.float64), "cycle_ok": ((B, n_cycles), np.uint8),
        "stance": ((B, 4, 3), np.float64), "selected": ((B, n_cycles, 4), SELECTED_DTYPE), "pose_status": ((B,), np.uint8),
        "selected_packed": ((B, n_cycles, 4), PACKED_DTYPE),
    }


class FpeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fpe error {code}: {msg}")
        self.code = code


def make_poses(xyz, gait=0, leg_search_radius=None, leg_polygon_kind=None):
    """Build an fpe_pose array from [B,3] positions (+ optional build-defined extensions)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    poses = np.zeros(xyz.shape[0], dtype=POSE_DTYPE)
    poses["position"] = xyz
    poses["gait"] = gait
    if leg_search_radius is not None:
        poses["leg_search_radius"] = leg_search_radius
    if leg_polygon_kind is not None:
        poses["leg_polygon_kind"] = leg_polygon_kind
    return poses


def make_strides(step_length, lateral_drift):
    """Build an fpe_stride array (one element per pose of a batch: plan(strides=...), plan_rank(strides=...)) from per-pose step
    lengths (kept as float32, the type of fpe_params.stepLength) and lateral drifts (float64); scalars broadcast."""
    step, drift = np.broadcast_arrays(np.asarray(step_length, dtype=np.float32), np.asarray(lateral_drift, dtype=np.float64))
    strides = np.zeros(step.size, dtype=STRIDE_DTYPE)
    strides["step_length"] = step.reshape(-1)
    strides["lateral_drift"] = drift.reshape(-1)
    return strides


def _strides_for(strides, B):
    strides = np.ascontiguousarray(strides, dtype=STRIDE_DTYPE)
    if strides.shape != (B,):
        raise ValueError(f"strides must hold one element per pose: shape {strides.shape}, {B} poses")
    return strides


def make_plan_states(params, poses=None, strides=None, feet=None, adjusted_y=0.0, cycle=0):
    """Build an fpe_plan_state array (plan_resume(states=...)).  From `poses` (and optional per-pose `strides`): what a plan of
    those poses starts from (fpe_plan_state_from_pose).  From `feet` ([B, 4, 2]: x / y of RF, RH, LH, LF — e.g. the request's four
    *_current_foothold points): all three tracks stand on them, with the given running drift and cycle index, scalars broadcast
    (fpe_plan_state_from_feet).  Pure host arithmetic: no engine, no GPU."""
    L = _capi.lib()
    if (poses is None) == (feet is None):
        raise ValueError("give either poses or feet")
    if feet is not None:
        feet = np.ascontiguousarray(feet, dtype=np.float64).reshape(-1, 4, 2)
        B = feet.shape[0]
        adj, cyc = np.broadcast_to(np.asarray(adjusted_y, np.float64), (B,)), np.broadcast_to(np.asarray(cycle, np.int32), (B,))
        states = np.zeros(B, dtype=PLAN_STATE_DTYPE)
        for b in range(B):
            rc = L.fpe_plan_state_from_feet(ptr(feet[b]), float(adj[b]), int(cyc[b]), ptr(states[b:b + 1]))
            if rc != _capi.FPE_OK:
                raise FpeError(rc, "fpe_plan_state_from_feet: non-finite value or cycle outside [0, 254]")
        return states
    params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(1)
    poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
    B = poses.shape[0]
    strides = _strides_for(strides, B) if strides is not None else None
    states = np.zeros(B, dtype=PLAN_STATE_DTYPE)
    for b in range(B):
        rc = L.fpe_plan_state_from_pose(ptr(params), ptr(poses[b:b + 1]), ptr(strides[b:b + 1]) if strides is not None else None,
                                        ptr(states[b:b + 1]))
        if rc != _capi.FPE_OK:
            raise FpeError(rc, "fpe_plan_state_from_pose: non-finite pose or stride")
    return states


def make_swing_queries(a, b, radius=0.0):
    """Build an fpe_swing_query array (swing_segments) from [n, 3] start points A and end points B (x, y, z) and per-segment capsule
    radii (float32; <= 0: the limits' radius, else params.footRadius); a scalar radius broadcasts."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    q = np.zeros(a.shape[0], dtype=_capi.SWING_QUERY_DTYPE)
    q["a"], q["b"], q["radius"] = a, b, radius
    return q


def make_swing_limits(max_lift=np.inf, max_rise=np.inf, max_length=np.inf, radius=0.0):
    """An fpe_swing_limits block: the limits behind the OVER bits (+infinity: no limit) and the capsule radius of segments that give
    none (<= 0: params.footRadius).  Pure host arithmetic: no engine, no GPU."""
    return _capi.SwingLimits(float(max_lift), float(max_rise), float(max_length), float(radius), 0)


def _swing_limits(limits):
    """None (the engine's defaults), a SwingLimits block, or a dict of make_swing_limits' keywords."""
    if limits is None or isinstance(limits, _capi.SwingLimits):
        return limits
    return make_swing_limits(**dict(limits))


def make_trunk_queries(feet, half_length=0.0, half_width=0.0):
    """Build an fpe_trunk_query array (trunk_stances) from [n, 4, 3] feet (RF, RH, LH, LF; x, y, z) and per-stance half extents of the
    body box (float32; <= 0: the limits' value, else half of params.length / params.width); scalars broadcast."""
    feet = np.asarray(feet, dtype=np.float64).reshape(-1, 4, 3)
    q = np.zeros(feet.shape[0], dtype=_capi.TRUNK_QUERY_DTYPE)
    q["feet"], q["half_length"], q["half_width"] = feet, half_length, half_width
    return q


def make_trunk_limits(min_clearance=-np.inf, max_slope_x=np.inf, max_slope_y=np.inf, ride_height=0.0, half_length=0.0, half_width=0.0):
    """An fpe_trunk_limits block: the limits behind UNDER_CLEARANCE / OVER_SLOPE (-/+infinity: no limit), the height of the body plane
    above the plane through the feet, and the box of stances that give none (<= 0: half of params.length / params.width).  Pure host
    arithmetic: no engine, no GPU."""
    return _capi.TrunkLimits(float(min_clearance), float(max_slope_x), float(max_slope_y), float(ride_height), float(half_length),
                             float(half_width), (C.c_int32 * 2)(0, 0))


def _trunk_limits(limits):
    """None (the engine's defaults), a TrunkLimits block, or a dict of make_trunk_limits' keywords."""
    if limits is None or isinstance(limits, _capi.TrunkLimits):
        return limits
    return make_trunk_limits(**dict(limits))


def make_margin_params(classes=_capi.MARGIN_LOW_CANDIDATE | _capi.MARGIN_UNKNOWN | _capi.MARGIN_OFF_MAP, reach_cells=8, min_margin=0.0):
    """An fpe_margin_params block: the FPE_MARGIN_* class bits that make a cell BAD, the reach in cells (1..31) and the limit in metres
    behind UNDER (0: no limit).  Pure host arithmetic: no engine, no GPU."""
    return _capi.MarginParams(int(classes), int(reach_cells), float(min_margin), (C.c_int32 * 2)(0, 0))


def _margin_params(mp):
    """None (the engine's defaults), a MarginParams block, or a dict of make_margin_params' keywords."""
    if mp is None or isinstance(mp, _capi.MarginParams):
        return mp
    return make_margin_params(**dict(mp))


CHECK_NAMES = {"swing": _capi.CHECK_SWING, "trunk": _capi.CHECK_TRUNK, "margin": _capi.CHECK_MARGIN, "unknown": _capi.CHECK_UNKNOWN}


def _check_bits(bits):
    """FPE_CHECK_* bits from an int or from names ("swing", "trunk", "margin", "unknown")."""
    if isinstance(bits, (int, np.integer)):
        return int(bits)
    return int(sum({CHECK_NAMES[k] for k in bits}))


def make_check_params(checks=("swing", "trunk", "margin"), reject=0, w_swing_over=10.0, w_lift=0.0, w_trunk_bad=10.0, w_margin_under=1.0,
                      w_unknown=1.0, swing=None, trunk=None, margin=None):
    """An fpe_check_params block (plan_rank_checked, check_plan_device): the enabled checks and the reject bits (ints of FPE_CHECK_*
    bits or names), the weights of the score's check terms, and each check's limits — None (that family's defaults: no limit), its
    make_*_limits / make_margin_params block, or a dict of those keywords.  Pure host arithmetic: no engine, no GPU."""
    cp = _capi.CheckParams()
    cp.checks, cp.reject = _check_bits(checks), _check_bits(reject)
    cp.w_swing_over, cp.w_lift, cp.w_trunk_bad = float(w_swing_over), float(w_lift), float(w_trunk_bad)
    cp.w_margin_under, cp.w_unknown, cp.reserved = float(w_margin_under), float(w_unknown), 0.0
    cp.swing = _swing_limits(swing) or make_swing_limits()
    cp.trunk = _trunk_limits(trunk) or make_trunk_limits()
    cp.margin = _margin_params(margin) or make_margin_params()
    return cp


def _check_params(cp):
    """None (the engine's defaults), a CheckParams block, or a dict of make_check_params' keywords."""
    if cp is None or isinstance(cp, _capi.CheckParams):
        return cp
    return make_check_params(**dict(cp))


def margin_metres(dist_sq, resolution):
    """The metric margin res * sqrt(dist_sq) of dist_sq values (any shape) as float64; +infinity where dist_sq is FPE_MARGIN_NONE."""
    d = np.asarray(dist_sq)
    return np.where(d == _capi.MARGIN_NONE, np.inf, float(resolution) * np.sqrt(d.astype(np.float64)))


# fpe_set_tuning's knobs whose engine default is not 0 (tuning() restores these after a with-block)
TUNING_DEFAULTS = {"service_opt_gate": 2, "service_overlap": 1, "service_poll": 1}


def _fill_products(po, addresses):
    """Set the fields of a PlanOut from {product name: address} — an array's ptr(), a device address, or 0 / None: not wanted."""
    for k, p in addresses.items():
        setattr(po, PRODUCT_FIELDS[k], p or None)
    return po


def _call_params(given, struct, defaults):
    """The parameter block of a ranking / beam call: None (the engine's defaults), a `struct` instance, or a dict of its fields to
    replace in `defaults()`."""
    if given is None or isinstance(given, struct):
        return given
    return defaults(**dict(given))


def _map_desc(rows, cols, resolution, position=(0.0, 0.0), start_index=(0, 0), storage_order="row"):
    return MapDesc(rows, cols, float(resolution), (C.c_double * 2)(*map(float, position)),
                   (C.c_int32 * 2)(*map(int, start_index)), 1 if storage_order == "row" else 0)


def make_map_update(shift, position, patches):
    """An fpe_map_update from raw patches (row0, col0, n_rows, n_cols, traversability address, elevation address, row_stride,
    col_stride), strides in floats.  More than UPDATE_MAX_PATCHES patches cannot be expressed: ValueError."""
    if len(patches) > _capi.UPDATE_MAX_PATCHES:
        raise ValueError(f"an update takes at most {_capi.UPDATE_MAX_PATCHES} patches")
    u = _capi.MapUpdate()
    u.shift[0], u.shift[1] = int(shift[0]), int(shift[1])
    u.position[0], u.position[1] = float(position[0]), float(position[1])
    u.n_patches = len(patches)
    for k, (row0, col0, n_rows, n_cols, t, e, rs, cs) in enumerate(patches):
        u.patch[k] = _capi.MapPatch(int(row0), int(col0), int(n_rows), int(n_cols), t, e, int(rs), int(cs))
    return u


def _host_patches(patches):
    """[(row0, col0, traversability, elevation), ...] with 2-D arrays or views of one shape (n_rows, n_cols) -> raw patches and the
    arrays they point into.  The strides are the arrays' own where both layers share one of the two forms of fpe_map_patch (row-
    or column-major with a pitch: a view into a message buffer goes as it is); anything else is copied to a packed array first."""
    raw, keep = [], []
    for row0, col0, trav, elev in patches:
        t, e = np.asarray(trav), np.asarray(elev)
        if t.ndim != 2 or t.shape != e.shape:
            raise ValueError("a patch is two 2-D arrays of one shape")
        n_rows, n_cols = t.shape
        rs, cs = (t.strides[0] // 4, t.strides[1] // 4) if n_rows and n_cols else (0, 0)
        direct = (t.dtype == np.float32 and e.dtype == np.float32 and t.strides == e.strides and t.strides[0] % 4 == 0 and t.strides[1] % 4 == 0
                  and ((cs == 1 and rs >= n_cols) or (rs == 1 and cs >= n_rows)))
        if not direct and n_rows and n_cols:
            t, e = np.ascontiguousarray(t, dtype=np.float32), np.ascontiguousarray(e, dtype=np.float32)
            rs, cs = n_cols, 1
        keep += [t, e]
        raw.append((row0, col0, n_rows, n_cols, t.ctypes.data, e.ctypes.data, rs, cs))
    return raw, keep


def _host_elevation_patches(patches):
    """[(row0, col0, elevation), ...] -> raw patches of an elevation-driven update (null traversability) and the arrays they point
    into; strides as in _host_patches."""
    raw, keep = _host_patches([(row0, col0, elev, elev) for row0, col0, elev in patches])
    return [(r0, c0, nr, nc, None, e, rs, cs) for r0, c0, nr, nc, _, e, rs, cs in raw], keep


def _info_dict(info):
    return {"reach_cells": int(info.reach_cells), "route": int(info.route), "dirty_cells": int(info.dirty_cells),
            "recomputed_cells": int(info.recomputed_cells)}


def filter_reach_cells(resolution, params=None):
    """fpe_filter_reach_cells: how many cells (Chebyshev) a changed elevation cell reaches into the traversability layer."""
    r = _capi.lib().fpe_filter_reach_cells(C.byref(params) if params is not None else None, float(resolution))
    if r < 0:
        raise FpeError(r, "fpe_filter_reach_cells: bad filter parameters or resolution")
    return r


def elevation_update_plan(rows, cols, resolution, shift, position, rects, params=None, want_mask=True):
    """fpe_elevation_update_plan (host arithmetic, no engine): the refusals and the dirty set of an elevation-driven update of a
    rows x cols map.  rects: [(row0, col0, n_rows, n_cols), ...] (packed row-major sources are assumed) or raw patches as for
    make_map_update.  Returns (info dict, dirty mask (rows, cols) uint8 or None); raises FpeError on a refusal."""
    one = np.zeros(1, np.float32)  # the plan reads no patch value: any non-null elevation address will do
    raw = [(p[0], p[1], p[2], p[3], None, one.ctypes.data, p[3], 1) if len(p) == 4 else p for p in rects]
    u = make_map_update(shift, position, raw)
    d = _map_desc(rows, cols, resolution)
    info = _capi.ElevationUpdateInfo()
    mask = np.zeros((rows, cols), np.uint8) if want_mask and rows > 0 and cols > 0 else None
    rc = _capi.lib().fpe_elevation_update_plan(C.byref(d), C.byref(params) if params is not None else None, C.byref(u), C.byref(info), ptr(mask))
    if rc != _capi.FPE_OK:
        raise FpeError(rc, "fpe_elevation_update_plan refused the update")
    return _info_dict(info), mask


def scan_params(**overrides):
    """fpe_scan_params_defaults, with any field replaced by a keyword."""
    sp = _capi.ScanParams()
    assert _capi.lib().fpe_scan_params_defaults(C.byref(sp)) == _capi.FPE_OK
    for k, v in overrides.items():
        if k not in dict(_capi.ScanParams._fields_):
            raise ValueError(f"unknown scan parameter {k!r}")
        setattr(sp, k, v)
    return sp


def make_scan(sensor_to_map, n_points, roi, point_stride=3):
    """An fpe_scan: the sensor-to-map transform (3 x 4, or 4 x 4 whose last row is dropped; row-major), the number of points, their
    stride in floats and the roi (row0, col0, n_rows, n_cols) of the state the scan may write."""
    t = np.asarray(sensor_to_map, dtype=np.float64)
    if t.shape == (4, 4):
        t = t[:3]
    if t.size != 12:
        raise ValueError("sensor_to_map is a 3 x 4 (or 4 x 4) matrix")
    s = _capi.Scan()
    s.sensor_to_map[:] = [float(x) for x in t.reshape(12)]
    s.n_points, s.point_stride = int(n_points), int(point_stride)
    s.roi[:] = [int(x) for x in roi]
    return s


def scan_validate(rows, cols, resolution, params, scan):
    """fpe_scan_validate (host arithmetic, no engine): the status a fuse of `scan` into a rows x cols state would be refused with,
    or FPE_OK.  `params` / `scan` may be None (a null argument)."""
    d = _map_desc(rows, cols, resolution)
    return _capi.lib().fpe_scan_validate(C.byref(d), C.byref(params) if params is not None else None, C.byref(scan) if scan is not None else None)


def scan_clear_params(**overrides):
    """fpe_scan_clear_params_defaults, with any field replaced by a keyword."""
    cp = _capi.ScanClearParams()
    assert _capi.lib().fpe_scan_clear_params_defaults(C.byref(cp)) == _capi.FPE_OK
    for k, v in overrides.items():
        if k not in dict(_capi.ScanClearParams._fields_):
            raise ValueError(f"unknown scan clear parameter {k!r}")
        setattr(cp, k, v)
    return cp


def scan_clear_validate(rows, cols, resolution, params, clear_params, scan):
    """fpe_scan_clear_validate (host arithmetic, no engine): the status a clear of `scan` in a rows x cols state would be refused
    with, or FPE_OK.  `params` / `clear_params` / `scan` may be None (a null argument)."""
    d = _map_desc(rows, cols, resolution)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    return _capi.lib().fpe_scan_clear_validate(C.byref(d), ref(params), ref(clear_params), ref(scan))


def scan_close_params(**overrides):
    """fpe_scan_close_params_defaults, with any field replaced by a keyword (reserved: a sequence of four)."""
    kp = _capi.ScanCloseParams()
    assert _capi.lib().fpe_scan_close_params_defaults(C.byref(kp)) == _capi.FPE_OK
    for k, v in overrides.items():
        if k not in dict(_capi.ScanCloseParams._fields_):
            raise ValueError(f"unknown scan close parameter {k!r}")
        if k == "reserved":
            kp.reserved[:] = [int(x) for x in v]
        else:
            setattr(kp, k, v)
    return kp


def make_scan_image(model, format, width, height, row_pitch=None, row_step=1, col_step=1, depth_scale=1.0, fx=1.0, fy=1.0, cx=0.0, cy=0.0,
                    row_dir=None, col_dir=None):
    """An fpe_scan_image.  model: "pinhole" / "spherical" (or the constant); format: "u16" / "f32".  row_dir / col_dir (spherical): a
    float32 array of (height, 2) / (width, 2) {cos, sin} for the host forms (kept alive by the descriptor), or a device address."""
    im = _capi.ScanImage()
    im.model = {"pinhole": _capi.SCAN_IMAGE_PINHOLE, "spherical": _capi.SCAN_IMAGE_SPHERICAL}.get(model, model)
    im.format = {"u16": _capi.SCAN_DEPTH_U16, "f32": _capi.SCAN_DEPTH_F32}.get(format, format)
    im.width, im.height = int(width), int(height)
    im.row_pitch = int(width if row_pitch is None else row_pitch)
    im.row_step, im.col_step = int(row_step), int(col_step)
    im.depth_scale, im.fx, im.fy, im.cx, im.cy = (float(x) for x in (depth_scale, fx, fy, cx, cy))
    keep = []
    for name, table in (("row_dir", row_dir), ("col_dir", col_dir)):
        if table is None or isinstance(table, int):
            setattr(im, name, table or None)
        else:
            t = np.ascontiguousarray(table, dtype=np.float32)
            keep.append(t)
            setattr(im, name, t.ctypes.data)
    im._keep = keep
    return im


def scan_image_selected(im):
    """(selected rows, selected columns) of a descriptor: n_sel is their product."""
    return -(-im.height // im.row_step), -(-im.width // im.col_step)


def scan_image_validate(rows, cols, resolution, params, clear_params, scan, im):
    """fpe_scan_image_validate (host arithmetic, no engine): the status an image form would be refused with, or FPE_OK.  Any of the
    four may be None (clear_params None: the fuse's refusals alone)."""
    d = _map_desc(rows, cols, resolution)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    return _capi.lib().fpe_scan_image_validate(C.byref(d), ref(params), ref(clear_params), ref(scan), ref(im))


def _image(image, im):
    """The host image as the library reads it: uint16 or float32 elements, at least (height - 1) * row_pitch + width of them."""
    a = np.ascontiguousarray(image, dtype=np.uint16 if im.format == _capi.SCAN_DEPTH_U16 else np.float32)
    if a.size < (im.height - 1) * im.row_pitch + im.width:
        raise ValueError("fewer elements than (height - 1) * row_pitch + width")
    return a


def scan_image_points(im, image):
    """fpe_scan_image_points (host only): the (n_sel, 3) float32 points of the image by the contract's rule."""
    a = _image(image, im)
    nr, nc = scan_image_selected(im)
    out = np.empty((nr * nc, 3), np.float32)
    rc = _capi.lib().fpe_scan_image_points(C.byref(im), ptr(a), ptr(out))
    if rc != _capi.FPE_OK:
        raise FpeError(rc, "fpe_scan_image_points refused the descriptor")
    return out


def _rect(rect):
    return None if rect is None else (C.c_int32 * 4)(*(int(x) for x in rect))


def scan_close_validate(rows, cols, resolution, close_params, rect):
    """fpe_scan_close_validate (host arithmetic, no engine): the status a close of `rect` = (row0, col0, n_rows, n_cols) of a
    rows x cols state would be refused with, or FPE_OK.  `close_params` / `rect` may be None (a null argument)."""
    d = _map_desc(rows, cols, resolution)
    return _capi.lib().fpe_scan_close_validate(C.byref(d), C.byref(close_params) if close_params is not None else None, _rect(rect))


class _Handle:
    """What an engine and a group of engines share: the handle's creation, close / __del__, and the status check.  A subclass names
    its three entry points."""
    _CREATE = _DESTROY = _LAST_ERROR = None

    def _create(self, *args, params=None):
        self._lib = _capi.lib()
        self._h = C.c_void_p()
        rc = getattr(self._lib, self._CREATE)(*args, C.byref(self._h))
        if rc != _capi.FPE_OK:
            msg = getattr(self._lib, self._LAST_ERROR)(None).decode()
            self._h = None
            if rc == _capi.FPE_E_NO_DEVICE:
                raise EngineUnavailable(f"{self._CREATE} failed: {msg} (the engine has no CPU fallback)")
            raise FpeError(rc, msg)
        self.params = _capi.params_yaml() if params is None else np.array(params, dtype=PARAMS_DTYPE).reshape(1)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != _capi.FPE_OK:
            raise FpeError(rc, getattr(self._lib, self._LAST_ERROR)(self._h).decode())


class FootholdPlanner(_Handle):
    """One engine per process per GPU."""
    _CREATE, _DESTROY, _LAST_ERROR = "fpe_create", "fpe_destroy", "fpe_last_error"

    def __init__(self, device_id=0, params=None):
        self._create(int(device_id), params=params)
        self.opt_params = _capi.opt_params_yaml()  # nlopt/* of the yaml
        self.device_id = int(device_id)
        self._tuning = {}  # last value set per knob (tuning() restores these, not zeros)

    def close(self):
        if getattr(self, "_h", None):
            for p in getattr(self, "_pinned", []):  # arrays from host_array() must not be used after close()
                self._lib.fpe_host_free(self._h, p)
            self._pinned = []
        super().close()

    # ---- map ingest (gridmapCallback, cpp:504-536) -------------------------------------------------
    def gridmapCallback(self, traversability, elevation, resolution, position=(0.0, 0.0), start_index=(0, 0),
                        storage_order="row"):
        """Upload both layers once to HBM.  `storage_order`: "row" ((rows, cols) C arrays) or
        "col" (grid_map_msgs column-major buffers, flat or (cols, rows))."""
        trav = np.ascontiguousarray(traversability, dtype=np.float32)
        elev = np.ascontiguousarray(elevation, dtype=np.float32)
        if storage_order == "row":
            rows, cols = trav.shape
        else:
            cols, rows = trav.shape
        d = _map_desc(rows, cols, resolution, position, start_index, storage_order)
        self._check(self._lib.fpe_upload_map(self._h, C.byref(d), ptr(trav), ptr(elev)))
        self.rows, self.cols, self.resolution = rows, cols, float(resolution)

    def upload_map_device(self, d_trav_ptr, d_elev_ptr, rows, cols, resolution, position=(0.0, 0.0), start_index=(0, 0),
                          storage_order="row", stream=None):
        d = _map_desc(rows, cols, resolution, position, start_index, storage_order)
        self._check(self._lib.fpe_upload_map_device(self._h, C.byref(d), C.c_void_p(d_trav_ptr), C.c_void_p(d_elev_ptr),
                                                    C.c_void_p(stream or 0)))
        self.rows, self.cols, self.resolution = rows, cols, float(resolution)

    def update_map(self, shift, position, patches=()):
        """fpe_update_map: the current snapshot shifted by `shift` = (sr, sc) whole cells (new cell (i, j) carries old cell
        (i + sr, j + sc); cells without a source are cleared to NaN), then `patches` = [(row0, col0, traversability, elevation), ...]
        written over it in order — host arrays or views of shape (n_rows, n_cols), read with their own strides.  `position`: the new
        map's getPosition().  Synchronous."""
        raw, keep = _host_patches(patches)
        u = make_map_update(shift, position, raw)
        self._check(self._lib.fpe_update_map(self._h, C.byref(u)))
        del keep

    def update_map_device(self, shift, position, patches=(), stream=None):
        """fpe_update_map_device: `patches` = [(row0, col0, n_rows, n_cols, d_traversability_ptr, d_elevation_ptr, row_stride,
        col_stride), ...] with DEVICE addresses and strides in floats; asynchronous on `stream`."""
        u = make_map_update(shift, position, list(patches))
        self._check(self._lib.fpe_update_map_device(self._h, C.byref(u), C.c_void_p(stream or 0)))

    # ---- elevation-driven updates: the producer's filters on the dirty region only (fpe_update_elevation*) ----------
    def update_elevation(self, shift, position, patches=(), params=None):
        """fpe_update_elevation: update_map with patches = [(row0, col0, elevation), ...] that carry the elevation only; the
        traversability of the cells whose input changed comes from the filter chain (`params`: a FilterParams, None = the
        defaults), every other cell's is carried by the shift.  Returns the call's info dict (elevation_update_plan's).  Synchronous."""
        raw, keep = _host_elevation_patches(patches)
        u = make_map_update(shift, position, raw)
        info = _capi.ElevationUpdateInfo()
        self._check(self._lib.fpe_update_elevation(self._h, C.byref(params) if params is not None else None, C.byref(u), C.byref(info)))
        del keep
        return _info_dict(info)

    def update_elevation_device(self, shift, position, patches=(), params=None, stream=None):
        """fpe_update_elevation_device: `patches` = [(row0, col0, n_rows, n_cols, d_elevation_ptr, row_stride, col_stride), ...] with
        DEVICE addresses and strides in floats; asynchronous on `stream`, no host wait."""
        raw = [(r0, c0, nr, nc, None, e, rs, cs) for r0, c0, nr, nc, e, rs, cs in patches]
        u = make_map_update(shift, position, raw)
        info = _capi.ElevationUpdateInfo()
        self._check(self._lib.fpe_update_elevation_device(self._h, C.byref(params) if params is not None else None, C.byref(u), C.byref(info),
                                                          C.c_void_p(stream or 0)))
        return _info_dict(info)

    def read_map_layers(self, traversability=True, elevation=True):
        """fpe_read_map_layers: the canonical layers of the current snapshot, bit for bit -> (traversability, elevation) as
        (rows, cols) arrays (None for a layer not asked for)."""
        g = self.map_info()
        t = np.empty((g["rows"], g["cols"]), np.float32) if traversability else None
        e = np.empty((g["rows"], g["cols"]), np.float32) if elevation else None
        self._check(self._lib.fpe_read_map_layers(self._h, ptr(t), ptr(e)))
        return t, e

    def read_map_layers_device(self, d_trav_ptr=0, d_elev_ptr=0, stream=None):
        """fpe_read_map_layers_device: the same copy into device buffers (0: not wanted), asynchronous on `stream`."""
        self._check(self._lib.fpe_read_map_layers_device(self._h, C.c_void_p(d_trav_ptr or 0), C.c_void_p(d_elev_ptr or 0), C.c_void_p(stream or 0)))

    # ---- the producer of the map (launch/mapping.launch:12-13) ----------------------
    def filter_params(self, **overrides):
        fp = _capi.FilterParams()
        self._check(self._lib.fpe_filter_params_defaults(C.byref(fp)))
        for k, v in overrides.items():
            setattr(fp, k, v)
        return fp

    def traversability_from_elevation(self, elevation, resolution, position=(0.0, 0.0), start_index=(0, 0), storage_order="row",
                                      params=None, want_layers=False):
        """Elevation layer (host array in the message's layout) -> traversability layer (rows x cols, canonical) through
        the device filters; with want_layers also the dict of all FPE_FILTER_LAYERS layers."""
        elev = np.ascontiguousarray(elevation, dtype=np.float32)
        rows, cols = elev.shape if storage_order == "row" else elev.shape[::-1]
        d = _map_desc(rows, cols, resolution, position, start_index, storage_order)
        fp = params if params is not None else self.filter_params()
        trav = np.empty((rows, cols), np.float32)
        layers = np.empty((len(_capi.FILTER_LAYERS), rows, cols), np.float32) if want_layers else None
        self._check(self._lib.fpe_traversability(self._h, C.byref(d), C.byref(fp), ptr(elev), ptr(trav),
                                                 ptr(layers) if want_layers else None))
        if want_layers:
            return trav, {name: layers[k] for k, name in enumerate(_capi.FILTER_LAYERS)}
        return trav

    def traversability_device(self, d_elev_ptr, d_trav_ptr, rows, cols, resolution, position=(0.0, 0.0), params=None,
                              d_layers_ptr=0, stream=None):
        """Device-resident form (canonical row-major layers), asynchronous on `stream`."""
        d = _map_desc(rows, cols, resolution, position)
        fp = params if params is not None else self.filter_params()
        self._check(self._lib.fpe_traversability_device(self._h, C.byref(d), C.byref(fp), C.c_void_p(d_elev_ptr),
                                                        C.c_void_p(d_trav_ptr), C.c_void_p(d_layers_ptr or 0), C.c_void_p(stream or 0)))

    # ---- scan fusion: point clouds into an elevation layer that never leaves HBM (fpe_scan_*) ------------------------
    def scan_state(self, rows, cols, resolution, position=(0.0, 0.0)):
        """fpe_scan_create: a ScanState of this engine, every cell unknown."""
        return ScanState(self, rows, cols, resolution, position)

    def map_info(self):
        d = MapDesc()
        self._check(self._lib.fpe_map_info(self._h, C.byref(d)))
        return {"rows": d.rows, "cols": d.cols, "resolution": d.resolution, "position": tuple(d.position)}

    def set_max_leg_search_radius(self, r):
        self._check(self._lib.fpe_set_max_leg_search_radius(self._h, np.float32(r)))

    def describe_plan(self, strides=False, resume=False):
        """Name and shape of the kernel a chained plan launches with the current parameters and map; strides=True: the kernel
        a plan with per-pose strides launches (fpe_describe_plan_strides); resume=True: the kernel a plan_resume call launches
        (fpe_describe_plan_resume)."""
        buf = C.create_string_buffer(256)
        describe = self._lib.fpe_describe_plan_resume if resume else (self._lib.fpe_describe_plan_strides if strides else self._lib.fpe_describe_plan)
        self._check(describe(self._h, ptr(self.params), buf, 256))
        return buf.value.decode()

    def set_tuning(self, **kw):
        """fpe_set_tuning: plan_group, literal_discs, no_mid_variant, no_bits, beam_check_waves, scan_merge, scan_clear_form, scan_clear_group, scan_close_form, service_opt_gate, service_overlap, service_poll (build-defined test / tuning knobs)."""
        for k, v in kw.items():
            self._check(self._lib.fpe_set_tuning(self._h, k.encode(), int(v)))
            self._tuning[k] = int(v)

    @contextlib.contextmanager
    def tuning(self, **kw):
        """Set knobs for the duration of a with-block, then restore the values they had through this object (a knob
        this object never set goes back to 0, the automatic default; knobs seeded from the environment in fpe_create are
        not visible here — set them through set_tuning instead when with-blocks are used)."""
        before = {k: self._tuning.get(k, TUNING_DEFAULTS.get(k, 0)) for k in kw}
        self.set_tuning(**kw)
        try:
            yield self
        finally:
            self.set_tuning(**before)

    # ---- pinned host arrays (fpe_host_alloc): results are written into them by DMA, no copy-out ----------
    def host_array(self, shape, dtype):
        """A numpy array over pinned host memory of the engine (kept alive by the planner until close())."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._check(self._lib.fpe_host_alloc(self._h, max(n, 1), C.byref(p)))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        buf = (C.c_ubyte * max(n, 1)).from_address(p.value)
        a = np.frombuffer(buf, dtype=np.uint8, count=n).view(dtype).reshape(shape)
        a[...] = np.zeros((), dtype)
        return a

    def plan_outputs(self, B, n_cycles, products=DEFAULT_PRODUCTS, pinned=False):
        shapes = product_shapes(B, n_cycles)
        if not pinned:
            return {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in products}
        # ONE pinned block, the products behind one another in the order of the engine's device arena (each rounded up to
        # 256 bytes as there): fpe_plan then moves neighbours without padding in between in one DMA transfer
        order = [k for k in PRODUCT_ORDER if k in products]
        sizes = [int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize for k in order]
        offs, total = [], 0
        for n in sizes:
            offs.append(total)
            total += (n + 255) & ~255
        arena = self.host_array((max(total, 1),), np.uint8)
        return {k: arena[o:o + n].view(shapes[k][1]).reshape(shapes[k][0]) for k, o, n in zip(order, offs, sizes)}

    # ---- chained plan, host buffers ------------------------------------------------------------------
    def plan(self, poses, n_cycles, products=DEFAULT_PRODUCTS, out=None, strides=None):
        """fpe_plan with host buffers.  `out`: a dict returned by an earlier call with the same shapes (timing loops
        reuse the arrays instead of allocating ~100 B per foothold per call).  `strides`: an fpe_stride array (make_strides),
        one element per pose — pose b is planned with ITS step length and lateral drift (fpe_plan_strides)."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        shapes = product_shapes(B, n_cycles)
        if out is None:
            out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in products}
        else:  # the arrays of `out` are the products asked for (whatever `products` says)
            products = tuple(k for k in PRODUCT_ORDER if k in out)
            assert len(products) == len(out), f"unknown product in out: {sorted(set(out) - set(products))}"
        # the checked argument block of an `out` dict is kept for its next use (timing loops call with the same arrays: comparing
        # seven structured dtypes and taking seven pointers costs more Python time than the engine needs for its launches)
        key = (id(out), B, int(n_cycles), products) + tuple(out[k].ctypes.data for k in products)
        cached = getattr(self, "_plan_out_cache", None)
        if cached is not None and cached[0] == key:
            po = cached[1]
        else:
            for k in products:
                assert out[k].shape == shapes[k][0] and out[k].dtype == shapes[k][1]
            po = _fill_products(PlanOut(), {k: ptr(out[k]) for k in products})
            self._plan_out_cache = (key, po, out)
        if strides is None:
            self._check(self._lib.fpe_plan(self._h, ptr(self.params), ptr(poses), B, int(n_cycles), C.byref(po)))
        else:
            self._check(self._lib.fpe_plan_strides(self._h, ptr(self.params), ptr(poses), ptr(_strides_for(strides, B)), B, int(n_cycles),
                                                   C.byref(po)))
        return out

    # ---- resumable plans (build-defined: fpe_plan_resume*) ------------------------------------------------
    RESUME_PRODUCTS = ("nominal", "centroid", "default", "cycle_ok", "selected")  # what a continuation can return by default

    def plan_resume(self, poses, n_cycles, states=None, strides=None, products=None, want_state=True):
        """fpe_plan_resume with host buffers: plan `n_cycles` more cycles of every pose from `states` (an fpe_plan_state array, one
        element per pose: make_plan_states, or the states an earlier call returned; None: start from the poses as plan() does) and
        return (products, states) — the state behind the last cycle, to resume from again (None with want_state=False).  Records
        are indexed by the call's own cycle count and carry gait_cycle_id = state.cycle + g.  A resumed call has no stance and no
        pose_status; `products` defaults to plan()'s set without them (with them when states is None)."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        if products is None:
            products = DEFAULT_PRODUCTS if states is None else self.RESUME_PRODUCTS
        unknown = set(products) - set(PRODUCT_ORDER)
        if unknown:
            raise ValueError(f"unknown plan products {sorted(unknown)}")
        if states is not None:
            states = np.ascontiguousarray(states, dtype=PLAN_STATE_DTYPE)
            if states.shape != (B,):
                raise ValueError(f"states must hold one element per pose: shape {states.shape}, {B} poses")
        shapes = product_shapes(B, n_cycles)
        out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in PRODUCT_ORDER if k in products}
        po = _fill_products(PlanOut(), {k: ptr(a) for k, a in out.items()})
        state_out = np.zeros(B, dtype=PLAN_STATE_DTYPE) if want_state else None
        self._check(self._lib.fpe_plan_resume(self._h, ptr(self.params), ptr(poses), ptr(_strides_for(strides, B)) if strides is not None else None,
                                              ptr(states), B, int(n_cycles), C.byref(po), ptr(state_out)))
        return out, state_out

    def plan_resume_device(self, d_poses_ptr, B, n_cycles, d_out, d_state_in_ptr=0, d_state_out_ptr=0, d_strides_ptr=0, stream=0):
        """fpe_plan_resume_device: `d_out` maps product names to device pointers; the state pointers are device arrays of B
        fpe_plan_state elements (0: none; the two may be the same array).  Asynchronous on `stream`."""
        po = _fill_products(PlanOut(), d_out)
        self._check(self._lib.fpe_plan_resume_device(self._h, ptr(self.params), C.c_void_p(d_poses_ptr), C.c_void_p(d_strides_ptr or 0) if d_strides_ptr else None,
                                                     C.c_void_p(d_state_in_ptr) if d_state_in_ptr else None, int(B), int(n_cycles), C.byref(po),
                                                     C.c_void_p(d_state_out_ptr) if d_state_out_ptr else None, C.c_void_p(stream or 0)))

    # ---- beam search over stride options on resumable plans (build-defined: fpe_plan_beam*) ---------------------------------
    BEAM_PRODUCTS = ("nominal", "centroid", "default", "cycle_ok", "selected", "selected_packed")  # what a beam's plans can return

    def plan_beam(self, poses, options, beam=None, states=None, products=("nominal", "cycle_ok")):
        """fpe_plan_beam with host buffers: for every root pose a beam search over the stride `options` (an fpe_stride array,
        make_strides) — S segments of k cycles, the W best continuations kept per root (`beam`: None for the defaults, a
        _capi.BeamParams, or a dict of its fields) — from `states` (one fpe_plan_state per root) or from the poses.  Returns {"path":
        uint8 [B, W, S] option indices, "score", "penalty": float64 [B, W], "n_live": int32 [B], "state": fpe_plan_state [B, W], and
        each requested product with the shapes of plan() for B * W poses and S * k cycles, reshaped to [B, W, ...]}; slot (b, w) is
        root b's w-th best plan, and slots w >= n_live[b] are left as allocated (zeros)."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        options = np.ascontiguousarray(options, dtype=STRIDE_DTYPE).reshape(-1)
        B, M = poses.shape[0], options.shape[0]
        unknown = set(products) - set(self.BEAM_PRODUCTS)
        if unknown:
            raise ValueError(f"a beam call has no products {sorted(unknown)}")
        if states is not None:
            states = np.ascontiguousarray(states, dtype=PLAN_STATE_DTYPE)
            if states.shape != (B,):
                raise ValueError(f"states must hold one element per pose: shape {states.shape}, {B} poses")
        bp = _call_params(beam, _capi.BeamParams, _capi.beam_params_defaults)
        shape = bp if bp is not None else _capi.beam_params_defaults()
        S, k, W = max(int(shape.segments), 1), max(int(shape.cycles_per_segment), 1), max(int(shape.width), 1)
        shapes = product_shapes(B * W, S * k)
        out = {q: np.zeros(shapes[q][0], dtype=shapes[q][1]) for q in PRODUCT_ORDER if q in products}
        out.update(path=np.zeros((B, W, S), np.uint8), score=np.zeros((B, W)), penalty=np.zeros((B, W)), n_live=np.zeros(B, np.int32),
                   state=np.zeros((B, W), PLAN_STATE_DTYPE))
        bo = _capi.BeamOut(ptr(out["n_live"]), ptr(out["score"]), ptr(out["penalty"]), ptr(out["path"]), ptr(out["state"]))
        _fill_products(bo.products, {q: ptr(out[q]) for q in products})
        self._check(self._lib.fpe_plan_beam(self._h, ptr(self.params), C.byref(bp) if bp is not None else None, ptr(poses), ptr(states), B,
                                            ptr(options), M, C.byref(bo)))
        for q in products:
            out[q] = out[q].reshape((B, W) + out[q].shape[1:])
        return out

    def plan_beam_device(self, d_poses_ptr, B, d_options_ptr, M, d_path_ptr, beam=None, d_state_in_ptr=0, d_n_live_ptr=0, d_score_ptr=0,
                         d_penalty_ptr=0, d_state_ptr=0, products=None, stream=0):
        """fpe_plan_beam_device: DEVICE pointers (0 / missing = not wanted), asynchronous on `stream`.  products: {product name:
        device pointer} with plan()'s shapes for B * W poses and S * k cycles."""
        bo = _capi.BeamOut(d_n_live_ptr or None, d_score_ptr or None, d_penalty_ptr or None, d_path_ptr or None, d_state_ptr or None)
        _fill_products(bo.products, products or {})
        bp = _call_params(beam, _capi.BeamParams, _capi.beam_params_defaults)
        self._check(self._lib.fpe_plan_beam_device(self._h, ptr(self.params), C.byref(bp) if bp is not None else None, C.c_void_p(d_poses_ptr),
                                                   C.c_void_p(d_state_in_ptr) if d_state_in_ptr else None, int(B), C.c_void_p(d_options_ptr), int(M),
                                                   C.byref(bo), C.c_void_p(stream or 0)))

    # ---- checked beam: the swing, trunk and margin checks folded into the beam's pruning (build-defined: fpe_plan_beam_checked*) ----
    def plan_beam_checked(self, poses, options, beam=None, checks=None, states=None, start_feet=None, products=("nominal", "cycle_ok")):
        """fpe_plan_beam_checked with host buffers: plan_beam with every candidate's path also reduced on the device to the enabled
        checks' summaries, which enter the score and the class in every segment.  `checks`: as in plan_rank_checked; start_feet:
        float64 [B, 4, 3] (x, y, z of RF, RH, LH, LF) where the roots' feet stand, or None (the plan's stance; with `states` a swing
        check needs them).  Returns plan_beam's dict — "penalty" and "score" hold the checked values — plus, with any check enabled,
        "base_penalty": float64 [B, W], "hit": uint8 [B, W] of FPE_CHECK_* bits, "feet": float64 [B, W, 4, 3] (the start_feet of a
        following call, with "state" as its states) and "swing_summary" / "trunk_summary" / "margin_summary" [B, W] for the enabled
        checks; slots w >= n_live[b] are left as allocated (zeros)."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        options = np.ascontiguousarray(options, dtype=STRIDE_DTYPE).reshape(-1)
        B, M = poses.shape[0], options.shape[0]
        unknown = set(products) - set(self.BEAM_PRODUCTS)
        if unknown:
            raise ValueError(f"a beam call has no products {sorted(unknown)}")
        if states is not None:
            states = np.ascontiguousarray(states, dtype=PLAN_STATE_DTYPE)
            if states.shape != (B,):
                raise ValueError(f"states must hold one element per pose: shape {states.shape}, {B} poses")
        if start_feet is not None:
            start_feet = np.ascontiguousarray(start_feet, dtype=np.float64)
            if start_feet.shape != (B, 4, 3):
                raise ValueError(f"start_feet must be [B, 4, 3]: shape {start_feet.shape}, {B} poses")
        bp = _call_params(beam, _capi.BeamParams, _capi.beam_params_defaults)
        shape = bp if bp is not None else _capi.beam_params_defaults()
        S, k, W = max(int(shape.segments), 1), max(int(shape.cycles_per_segment), 1), max(int(shape.width), 1)
        shapes = product_shapes(B * W, S * k)
        out = {q: np.zeros(shapes[q][0], dtype=shapes[q][1]) for q in PRODUCT_ORDER if q in products}
        out.update(path=np.zeros((B, W, S), np.uint8), score=np.zeros((B, W)), penalty=np.zeros((B, W)), n_live=np.zeros(B, np.int32),
                   state=np.zeros((B, W), PLAN_STATE_DTYPE))
        bo = _capi.BeamOut(ptr(out["n_live"]), ptr(out["score"]), ptr(out["penalty"]), ptr(out["path"]), ptr(out["state"]))
        _fill_products(bo.products, {q: ptr(out[q]) for q in products})
        cp = _check_params(checks)
        on = cp.checks if cp is not None else _capi.CHECK_SWING | _capi.CHECK_TRUNK | _capi.CHECK_MARGIN
        co = _capi.BeamCheckOut()
        if on:
            out.update(base_penalty=np.zeros((B, W)), hit=np.zeros((B, W), np.uint8), feet=np.zeros((B, W, 4, 3)))
            co.base_penalty, co.hit, co.feet = ptr(out["base_penalty"]), ptr(out["hit"]), ptr(out["feet"])
            for name, bit, dt in (("swing", _capi.CHECK_SWING, _capi.SWING_SUMMARY_DTYPE), ("trunk", _capi.CHECK_TRUNK, _capi.TRUNK_SUMMARY_DTYPE),
                                  ("margin", _capi.CHECK_MARGIN, _capi.MARGIN_SUMMARY_DTYPE)):
                if on & bit:
                    out[name + "_summary"] = np.zeros((B, W), dt)
                    setattr(co, name, ptr(out[name + "_summary"]))
        self._check(self._lib.fpe_plan_beam_checked(self._h, ptr(self.params), C.byref(bp) if bp is not None else None,
                                                    C.byref(cp) if cp is not None else None, ptr(poses), ptr(states), ptr(start_feet), B,
                                                    ptr(options), M, C.byref(bo), C.byref(co)))
        for q in products:
            out[q] = out[q].reshape((B, W) + out[q].shape[1:])
        return out

    def plan_beam_checked_device(self, d_poses_ptr, B, d_options_ptr, M, d_path_ptr, beam=None, checks=None, d_state_in_ptr=0,
                                 d_start_feet_ptr=0, d_n_live_ptr=0, d_score_ptr=0, d_penalty_ptr=0, d_state_ptr=0, products=None,
                                 check_out=None, stream=0):
        """fpe_plan_beam_checked_device: plan_beam_device's arguments plus `checks` (as plan_rank_checked), the roots' start feet
        ([B, 4, 3] doubles; 0: the stance) and check_out: a dict {"swing" | "trunk" | "margin" | "base_penalty" | "hit" | "feet":
        device pointer} of the per-slot check outputs wanted (None: none)."""
        bo = _capi.BeamOut(d_n_live_ptr or None, d_score_ptr or None, d_penalty_ptr or None, d_path_ptr or None, d_state_ptr or None)
        _fill_products(bo.products, products or {})
        bp = _call_params(beam, _capi.BeamParams, _capi.beam_params_defaults)
        cp = _check_params(checks)
        co = _capi.BeamCheckOut(**{k: (v or None) for k, v in check_out.items()}) if check_out is not None else None
        self._check(self._lib.fpe_plan_beam_checked_device(self._h, ptr(self.params), C.byref(bp) if bp is not None else None,
                                                           C.byref(cp) if cp is not None else None, C.c_void_p(d_poses_ptr),
                                                           C.c_void_p(d_state_in_ptr) if d_state_in_ptr else None,
                                                           C.c_void_p(d_start_feet_ptr) if d_start_feet_ptr else None, int(B),
                                                           C.c_void_p(d_options_ptr), int(M), C.byref(bo),
                                                           C.byref(co) if co is not None else None, C.c_void_p(stream or 0)))

    # ---- chained plan, device-resident (torch tensors / raw pointers) ----------------------------------
    def plan_device(self, d_poses_ptr, B, n_cycles, d_nominal_ptr=0, d_centroid_ptr=0, d_default_ptr=0,
                    d_cycle_ok_ptr=0, d_stance_ptr=0, stream=0, d_selected_ptr=0, d_pose_status_ptr=0, d_selected_packed_ptr=0,
                    d_strides_ptr=0):
        """d_strides_ptr: device array of B fpe_stride elements (fpe_plan_strides_device), or 0 for fpe_plan_device."""
        po = PlanOut(d_nominal_ptr or None, d_centroid_ptr or None, d_default_ptr or None, d_cycle_ok_ptr or None,
                     d_stance_ptr or None, d_selected_ptr or None, d_pose_status_ptr or None, d_selected_packed_ptr or None)
        if not d_strides_ptr:
            self._check(self._lib.fpe_plan_device(self._h, ptr(self.params), C.c_void_p(d_poses_ptr), int(B), int(n_cycles),
                                                  C.byref(po), C.c_void_p(stream or 0)))
        else:
            self._check(self._lib.fpe_plan_strides_device(self._h, ptr(self.params), C.c_void_p(d_poses_ptr), C.c_void_p(d_strides_ptr),
                                                          int(B), int(n_cycles), C.byref(po), C.c_void_p(stream or 0)))

    # ---- plan a batch and rank it on the device (build-defined: fpe_plan_rank*) ---------------------------------------------
    def plan_rank(self, poses, n_cycles, K, rank=None, products=("nominal", "cycle_ok", "stance"), summary=True, strides=None):
        """fpe_plan_rank with host buffers: plans the batch, scores every pose on the device and returns {"best": int32 [K] pose
        indices, best first, "n_class0": int, "summary": POSE_SUMMARY_DTYPE [B] and "score": float64 [B] (with summary=True),
        and each requested product of the K chosen poses, slot k = pose best[k]} — shapes of plan() with B replaced by K.
        `strides`: as in plan() (fpe_plan_rank_strides) — the candidates of one ranking may differ in stride."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B, K = poses.shape[0], int(K)
        unknown = set(products) - set(PRODUCT_ORDER)
        if unknown:
            raise ValueError(f"unknown plan products {sorted(unknown)}")
        shapes = product_shapes(max(K, 0), n_cycles)
        out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in PRODUCT_ORDER if k in products}
        best = np.zeros(max(K, 0), np.int32)
        n0 = np.zeros(1, np.int32)
        ro = RankOut(None, None, ptr(best), ptr(n0))
        if summary:
            out["summary"] = np.zeros(B, _capi.POSE_SUMMARY_DTYPE)
            out["score"] = np.zeros(B, np.float64)
            ro.summary, ro.score = ptr(out["summary"]), ptr(out["score"])
        _fill_products(ro.best_products, {k: ptr(out[k]) for k in products})
        rp = _call_params(rank, _capi.RankParams, _capi.rank_params_defaults)
        if strides is None:
            self._check(self._lib.fpe_plan_rank(self._h, ptr(self.params), C.byref(rp) if rp is not None else None, ptr(poses), B,
                                                int(n_cycles), K, C.byref(ro)))
        else:
            self._check(self._lib.fpe_plan_rank_strides(self._h, ptr(self.params), C.byref(rp) if rp is not None else None, ptr(poses),
                                                        ptr(_strides_for(strides, B)), B, int(n_cycles), K, C.byref(ro)))
        out["best"], out["n_class0"] = best, int(n0[0])
        return out

    def plan_rank_device(self, d_poses_ptr, B, n_cycles, K, d_best_ptr, rank=None, d_summary_ptr=0, d_score_ptr=0, d_n_class0_ptr=0,
                         best_products=None, full=None, stream=0, d_strides_ptr=0):
        """Device form: DEVICE pointers (0 / missing = not wanted), asynchronous on `stream`.  best_products / full: dicts
        {product name: device pointer} of the K-slot compacted products and of the un-compacted products of all B poses."""
        ro = RankOut(d_summary_ptr or None, d_score_ptr or None, d_best_ptr or None, d_n_class0_ptr or None)
        _fill_products(ro.best_products, best_products or {})
        fo = _fill_products(PlanOut(), full) if full is not None else None
        rp = _call_params(rank, _capi.RankParams, _capi.rank_params_defaults)
        self._check(self._lib.fpe_plan_rank_strides_device(self._h, ptr(self.params), C.byref(rp) if rp is not None else None,
                                                           C.c_void_p(d_poses_ptr), C.c_void_p(d_strides_ptr or 0), int(B), int(n_cycles),
                                                           int(K), C.byref(fo) if fo is not None else None, C.byref(ro),
                                                           C.c_void_p(stream or 0)))

    # ---- checked ranking: the swing, trunk and margin checks folded into the pick (build-defined: fpe_plan_rank_checked*) ----
    def plan_rank_checked(self, poses, n_cycles, K, rank=None, checks=None, products=("nominal", "cycle_ok", "stance"), summary=True,
                          strides=None):
        """fpe_plan_rank_checked with host buffers: plan_rank with every pose's plan also reduced on the device to the enabled
        checks' summaries, which enter the score and the class.  `checks`: None (all three checks with their default limits, no
        reject bit), make_check_params(...) or a dict of its keywords.  Returns plan_rank's dict — "score" is the checked score —
        plus (summary=True) "base_score": float64 [B], "hit": uint8 [B] of FPE_CHECK_* bits, and "swing_summary" / "trunk_summary" /
        "margin_summary" [B] for the enabled checks."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B, K = poses.shape[0], int(K)
        unknown = set(products) - set(PRODUCT_ORDER)
        if unknown:
            raise ValueError(f"unknown plan products {sorted(unknown)}")
        shapes = product_shapes(max(K, 0), n_cycles)
        out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in PRODUCT_ORDER if k in products}
        best = np.zeros(max(K, 0), np.int32)
        n0 = np.zeros(1, np.int32)
        ro = RankOut(None, None, ptr(best), ptr(n0))
        _fill_products(ro.best_products, {k: ptr(out[k]) for k in products})
        cp = _check_params(checks)
        on = cp.checks if cp is not None else _capi.CHECK_SWING | _capi.CHECK_TRUNK | _capi.CHECK_MARGIN
        co = _capi.CheckOut()
        if summary:
            out["summary"] = np.zeros(B, _capi.POSE_SUMMARY_DTYPE)
            out["score"], out["base_score"], out["hit"] = np.zeros(B, np.float64), np.zeros(B, np.float64), np.zeros(B, np.uint8)
            ro.summary, ro.score = ptr(out["summary"]), ptr(out["score"])
            co.base_score, co.hit = ptr(out["base_score"]), ptr(out["hit"])
            for name, bit, dt in (("swing", _capi.CHECK_SWING, _capi.SWING_SUMMARY_DTYPE), ("trunk", _capi.CHECK_TRUNK, _capi.TRUNK_SUMMARY_DTYPE),
                                  ("margin", _capi.CHECK_MARGIN, _capi.MARGIN_SUMMARY_DTYPE)):
                if on & bit:
                    out[name + "_summary"] = np.zeros(B, dt)
                    setattr(co, name, ptr(out[name + "_summary"]))
        rp = _call_params(rank, _capi.RankParams, _capi.rank_params_defaults)
        self._check(self._lib.fpe_plan_rank_checked(self._h, ptr(self.params), C.byref(rp) if rp is not None else None,
                                                    C.byref(cp) if cp is not None else None, ptr(poses),
                                                    ptr(_strides_for(strides, B)) if strides is not None else None, B, int(n_cycles), K,
                                                    C.byref(ro), C.byref(co)))
        out["best"], out["n_class0"] = best, int(n0[0])
        return out

    def plan_rank_checked_device(self, d_poses_ptr, B, n_cycles, K, d_best_ptr, rank=None, checks=None, d_summary_ptr=0, d_score_ptr=0,
                                 d_n_class0_ptr=0, best_products=None, full=None, check_out=None, stream=0, d_strides_ptr=0):
        """Device form: plan_rank_device's arguments plus `checks` (as plan_rank_checked) and check_out: a dict {"swing" | "trunk" |
        "margin" | "base_score" | "hit": device pointer} of the per-pose check outputs wanted (None: none)."""
        ro = RankOut(d_summary_ptr or None, d_score_ptr or None, d_best_ptr or None, d_n_class0_ptr or None)
        _fill_products(ro.best_products, best_products or {})
        fo = _fill_products(PlanOut(), full) if full is not None else None
        rp = _call_params(rank, _capi.RankParams, _capi.rank_params_defaults)
        cp = _check_params(checks)
        co = _capi.CheckOut(**{k: (v or None) for k, v in check_out.items()}) if check_out is not None else None
        self._check(self._lib.fpe_plan_rank_checked_device(self._h, ptr(self.params), C.byref(rp) if rp is not None else None,
                                                           C.byref(cp) if cp is not None else None, C.c_void_p(d_poses_ptr),
                                                           C.c_void_p(d_strides_ptr or 0), int(B), int(n_cycles), int(K),
                                                           C.byref(fo) if fo is not None else None, C.byref(ro),
                                                           C.byref(co) if co is not None else None, C.c_void_p(stream or 0)))

    def check_plan_device(self, d_nominal_ptr, d_cycle_ok_ptr, B, n_cycles, check_out, checks=None, d_stance_ptr=0, d_start_feet_ptr=0,
                          stream=0):
        """fpe_check_plan_device: the check stage alone on DEVICE pointers to a plan's products as a plan call on `stream` left them
        (the start feet: [B, 4, 3] doubles; 0: the stance product, d_stance_ptr).  check_out: as in plan_rank_checked_device, without
        "base_score" — the stage computes no score."""
        po = _fill_products(PlanOut(), {"nominal": d_nominal_ptr, "cycle_ok": d_cycle_ok_ptr, "stance": d_stance_ptr})
        cp = _check_params(checks)
        co = _capi.CheckOut(**{k: (v or None) for k, v in check_out.items()})
        self._check(self._lib.fpe_check_plan_device(self._h, ptr(self.params), C.byref(cp) if cp is not None else None, C.byref(po),
                                                    C.c_void_p(d_start_feet_ptr or 0), int(B), int(n_cycles), C.byref(co),
                                                    C.c_void_p(stream or 0)))

    # ---- the opt track of a batch (cpp:913-1319, 1485-1568; build-defined optimiser) ---------------------------
    def plan_opt(self, poses, n_cycles, cycle_ok=None):
        """fpe_plan_opt with host buffers; cycle_ok: the nominal plan's flags [B, n_cycles] (None: the engine plans first).
        Returns {"footholds" [B, n, 4], "cycles" [B, n], "gate_fail_cycle" [B], "rows_after" [B, 2]}."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        out = {"footholds": np.zeros((B, n_cycles, 4), OPT_FOOTHOLD_DTYPE), "cycles": np.zeros((B, n_cycles), OPT_CYCLE_DTYPE),
               "gate_fail_cycle": np.zeros(B, np.uint8), "rows_after": np.zeros((B, 2), np.float64)}
        ok = None if cycle_ok is None else np.ascontiguousarray(cycle_ok, dtype=np.uint8).reshape(B, n_cycles)
        oo = OptOut(ptr(out["footholds"]), ptr(out["cycles"]), ptr(out["gate_fail_cycle"]), ptr(out["rows_after"]))
        self._check(self._lib.fpe_plan_opt(self._h, ptr(self.params), ptr(self.opt_params), ptr(poses), B, int(n_cycles), ptr(ok),
                                           C.byref(oo)))
        return out

    def plan_opt_device(self, d_poses_ptr, B, n_cycles, d_cycle_ok_ptr, d_footholds_ptr=0, d_cycles_ptr=0, d_gate_ptr=0, stream=0):
        oo = OptOut(d_footholds_ptr or None, d_cycles_ptr or None, d_gate_ptr or None)
        self._check(self._lib.fpe_plan_opt_device(self._h, ptr(self.params), ptr(self.opt_params), C.c_void_p(d_poses_ptr), int(B),
                                                  int(n_cycles), C.c_void_p(d_cycle_ok_ptr), C.byref(oo), C.c_void_p(stream or 0)))

    # ---- open-loop per-leg search (checkFoothold, cpp:2001-2036) -----------------------------------------
    def checkFoothold(self, queries):
        queries = np.ascontiguousarray(queries, dtype=QUERY_DTYPE)
        out = np.zeros(queries.shape[0], dtype=FOOTHOLD_DTYPE)
        self._check(self._lib.fpe_search_legs(self._h, ptr(self.params), ptr(queries), queries.shape[0], ptr(out)))
        return out

    def search_legs_device(self, d_queries_ptr, n, d_out_ptr, stream=0):
        self._check(self._lib.fpe_search_legs_device(self._h, ptr(self.params), C.c_void_p(d_queries_ptr), int(n),
                                                     C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)))

    # ---- dense foothold map: checkDefaultFoothold / checkCirclePolygonFoothold / getFootholdMeanHeight at every cell centre --
    @staticmethod
    def _roi(roi):
        return None if roi is None else np.ascontiguousarray(roi, dtype=np.int32).reshape(4)

    # the dense maps: out struct of the C ABI (its field names are the product names) and per product (dtype, trailing shape)
    # behind [n_rows, n_cols]
    _DENSE = {"foothold-map": (FootholdMapOut, {"flags": (np.uint8, ()), "height": (np.float32, ())}),
              "foothold-snap": (FootholdSnapOut, {"offset": (np.int8, (2,)), "source": (np.uint8, ()), "z": (np.float32, ())}),
              "centroid-map": (CentroidMapOut, {"code": (np.uint8, ()), "offset": (np.int8, (2,)), "z": (np.float32, ())}),
              "margin-map": (_capi.MarginMapOut, {"dist_sq": (np.uint16, ()), "nearest": (np.int8, (2,))})}

    @classmethod
    def _dense_out(cls, what, **addresses):
        """The out struct of a dense map from {product: address} (host or device; 0 / None / missing = product not wanted)."""
        struct = cls._DENSE[what][0]
        return struct(*(addresses.get(name) or None for name, _ in struct._fields_))

    def _dense_outputs(self, what, roi, products):
        """The region as the C ABI takes it (None = the whole map), one uninitialised array per requested product of a dense
        map, and the out struct that points at them."""
        table = self._DENSE[what][1]
        unknown = set(products) - set(table)
        if unknown:
            raise ValueError(f"unknown {what} products {sorted(unknown)}")
        r = self._roi(roi)
        if r is not None:
            shape = (max(int(r[2]), 0), max(int(r[3]), 0))
        else:
            info = self.map_info()
            shape = (info["rows"], info["cols"])
        out = {k: np.empty(shape + tail, dtype) for k, (dtype, tail) in table.items() if k in products}
        return r, out, self._dense_out(what, **{k: a.ctypes.data for k, a in out.items()})

    def foothold_map(self, roi=None, products=("flags", "height")):
        """fpe_foothold_map on the current map: {"flags": uint8 [n_rows, n_cols] FPE_FMAP_* bits, "height": float32
        [n_rows, n_cols]} for the requested products.  roi = (row0, col0, n_rows, n_cols) in canonical indices; None = the
        whole map."""
        r, out, mo = self._dense_outputs("foothold-map", roi, products)
        self._check(self._lib.fpe_foothold_map(self._h, ptr(self.params), ptr(r), C.byref(mo)))
        return out

    def foothold_map_device(self, d_flags_ptr, d_height_ptr, roi=None, stream=0):
        """Device form: DEVICE pointers (0 = product not wanted), asynchronous on `stream`."""
        r = self._roi(roi)
        mo = self._dense_out("foothold-map", flags=d_flags_ptr, height=d_height_ptr)
        self._check(self._lib.fpe_foothold_map_device(self._h, ptr(self.params), ptr(r), C.byref(mo), C.c_void_p(stream or 0)))

    # ---- dense snap map: checkFoothold's landing cell for every cell centre -----------------------------------------------
    _POLYGONS = {"rectangle": 0, "hexagon": 1}

    @classmethod
    def _polygon_kind(cls, polygon):
        if isinstance(polygon, str):
            if polygon not in cls._POLYGONS:
                raise ValueError(f"unknown search polygon {polygon!r}")
            return cls._POLYGONS[polygon]
        return int(polygon)  # a raw polygon_kind: the engine checks it

    def foothold_snap(self, roi=None, search_radius=None, polygon="rectangle", products=("offset", "source", "z")):
        """fpe_foothold_snap on the current map: {"offset": int8 [n_rows, n_cols, 2] (di, dj) of the landing cell, "source":
        uint8 [n_rows, n_cols] (0 default hit, 1 spiral candidate, 2 none), "z": float32 [n_rows, n_cols]} for the requested
        products.  roi as in foothold_map; search_radius None = params.searchRadius; polygon "rectangle" | "hexagon"."""
        r, out, so = self._dense_outputs("foothold-snap", roi, products)
        self._check(self._lib.fpe_foothold_snap(self._h, ptr(self.params), ptr(r), float(search_radius or 0.0),
                                                self._polygon_kind(polygon), C.byref(so)))
        return out

    def foothold_snap_device(self, d_offset_ptr, d_source_ptr, d_z_ptr, roi=None, search_radius=None, polygon="rectangle",
                             stream=0):
        """Device form: DEVICE pointers (0 = product not wanted), asynchronous on `stream`."""
        r = self._roi(roi)
        so = self._dense_out("foothold-snap", offset=d_offset_ptr, source=d_source_ptr, z=d_z_ptr)
        self._check(self._lib.fpe_foothold_snap_device(self._h, ptr(self.params), ptr(r), float(search_radius or 0.0),
                                                       self._polygon_kind(polygon), C.byref(so), C.c_void_p(stream or 0)))

    # ---- open-loop centroid method and the dense centroid map (checkFootholdUseCentroidMethod, cpp:1605-1997) ---------------
    def centroid_legs(self, queries):
        """fpe_centroid_legs: one CENTROID_DTYPE record per CENTROID_QUERY_DTYPE query (cx, cy, search_radius <= 0 =
        params.searchRadius)."""
        queries = np.ascontiguousarray(queries, dtype=CENTROID_QUERY_DTYPE).reshape(-1)
        out = np.zeros(queries.shape[0], dtype=CENTROID_DTYPE)
        self._check(self._lib.fpe_centroid_legs(self._h, ptr(self.params), ptr(queries), queries.shape[0], ptr(out)))
        return out

    def centroid_legs_device(self, d_queries_ptr, n, d_out_ptr, stream=0):
        """Device form: DEVICE pointers to n queries and n records, asynchronous on `stream`."""
        self._check(self._lib.fpe_centroid_legs_device(self._h, ptr(self.params), C.c_void_p(d_queries_ptr), int(n),
                                                       C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)))

    def centroid_map(self, roi=None, search_radius=None, products=("code", "offset", "z")):
        """fpe_centroid_map on the current map: {"code": uint8 [n_rows, n_cols] (0..6), "offset": int8 [n_rows, n_cols, 2]
        (row - i, col - j) of the landing cell, "z": float32 [n_rows, n_cols]} for the requested products.  roi as in
        foothold_map; search_radius None = params.searchRadius."""
        r, out, co = self._dense_outputs("centroid-map", roi, products)
        self._check(self._lib.fpe_centroid_map(self._h, ptr(self.params), ptr(r), float(search_radius or 0.0), C.byref(co)))
        return out

    def centroid_map_device(self, d_code_ptr, d_offset_ptr, d_z_ptr, roi=None, search_radius=None, stream=0):
        """Device form: DEVICE pointers (0 = product not wanted), asynchronous on `stream`."""
        r = self._roi(roi)
        co = self._dense_out("centroid-map", code=d_code_ptr, offset=d_offset_ptr, z=d_z_ptr)
        self._check(self._lib.fpe_centroid_map_device(self._h, ptr(self.params), ptr(r), float(search_radius or 0.0), C.byref(co),
                                                      C.c_void_p(stream or 0)))

    # ---- swing checks: each planned step against the elevation layer (build-defined: fpe_swing_*) ---------------------------
    def swing_segments(self, queries, limits=None):
        """fpe_swing_segments: one SWING_RECORD_DTYPE record per SWING_QUERY_DTYPE query (make_swing_queries) on the current map.
        `limits`: None (no limit, radius params.footRadius), make_swing_limits(...) or a dict of its keywords."""
        queries = np.ascontiguousarray(queries, dtype=_capi.SWING_QUERY_DTYPE).reshape(-1)
        out = np.zeros(queries.shape[0], dtype=_capi.SWING_RECORD_DTYPE)
        sl = _swing_limits(limits)
        self._check(self._lib.fpe_swing_segments(self._h, ptr(self.params), C.byref(sl) if sl is not None else None, ptr(queries),
                                                 queries.shape[0], ptr(out)))
        return out

    def swing_segments_device(self, d_queries_ptr, n, d_out_ptr, limits=None, stream=0):
        """Device form: DEVICE pointers to n queries and n records, asynchronous on `stream`."""
        sl = _swing_limits(limits)
        self._check(self._lib.fpe_swing_segments_device(self._h, ptr(self.params), C.byref(sl) if sl is not None else None,
                                                        C.c_void_p(d_queries_ptr), int(n), C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)))

    def plan_swing(self, poses, n_cycles, limits=None, strides=None, products=("nominal", "cycle_ok", "stance"), summary=True):
        """fpe_swing_plan with host buffers: plans the batch as plan() does (strides: as there) and checks every planned step against
        the elevation layer in the same call.  Returns the requested plan products plus "swing": SWING_RECORD_DTYPE [B, n_cycles, 4],
        "swing_length": float64 sqrt of its length_sq, and (summary=True) "swing_summary": SWING_SUMMARY_DTYPE [B].  The start feet
        are the plan's stance, which carries the pose's z."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        unknown = set(products) - set(PRODUCT_ORDER)
        if unknown:
            raise ValueError(f"unknown plan products {sorted(unknown)}")
        shapes = product_shapes(B, n_cycles)
        out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in PRODUCT_ORDER if k in products}
        po = _fill_products(PlanOut(), {k: ptr(out[k]) for k in out})
        out["swing"] = np.zeros((B, n_cycles, 4), _capi.SWING_RECORD_DTYPE)
        so = _capi.SwingOut(ptr(out["swing"]), None)
        if summary:
            out["swing_summary"] = np.zeros(B, _capi.SWING_SUMMARY_DTYPE)
            so.summary = ptr(out["swing_summary"])
        sl = _swing_limits(limits)
        self._check(self._lib.fpe_swing_plan(self._h, ptr(self.params), C.byref(sl) if sl is not None else None, ptr(poses),
                                             ptr(_strides_for(strides, B)) if strides is not None else None, B, int(n_cycles),
                                             C.byref(po), C.byref(so)))
        out["swing_length"] = np.sqrt(out["swing"]["length_sq"])
        return out

    def swing_plan_device(self, d_nominal_ptr, d_cycle_ok_ptr, B, n_cycles, d_records_ptr=0, d_summary_ptr=0, d_stance_ptr=0,
                          d_start_feet_ptr=0, limits=None, stream=0):
        """fpe_swing_plan_device: DEVICE pointers to a plan's nominal and cycle_ok products as a plan call on `stream` left them, the
        start feet ([B, 4, 3] doubles; 0: the plan's stance product, d_stance_ptr) and the outputs (0 = not wanted)."""
        po = _fill_products(PlanOut(), {"nominal": d_nominal_ptr, "cycle_ok": d_cycle_ok_ptr, "stance": d_stance_ptr})
        so = _capi.SwingOut(d_records_ptr or None, d_summary_ptr or None)
        sl = _swing_limits(limits)
        self._check(self._lib.fpe_swing_plan_device(self._h, ptr(self.params), C.byref(sl) if sl is not None else None, C.byref(po),
                                                    C.c_void_p(d_start_feet_ptr or 0), int(B), int(n_cycles), C.byref(so),
                                                    C.c_void_p(stream or 0)))

    # ---- trunk checks: each planned stance's body box against the elevation layer (build-defined: fpe_trunk_*) -------------
    def trunk_stances(self, queries, limits=None):
        """fpe_trunk_stances: one TRUNK_RECORD_DTYPE record per TRUNK_QUERY_DTYPE query (make_trunk_queries) on the current map.
        `limits`: None (no limit, ride height 0, the box of params.length x params.width), make_trunk_limits(...) or a dict of its
        keywords."""
        queries = np.ascontiguousarray(queries, dtype=_capi.TRUNK_QUERY_DTYPE).reshape(-1)
        out = np.zeros(queries.shape[0], dtype=_capi.TRUNK_RECORD_DTYPE)
        tl = _trunk_limits(limits)
        self._check(self._lib.fpe_trunk_stances(self._h, ptr(self.params), C.byref(tl) if tl is not None else None, ptr(queries),
                                                queries.shape[0], ptr(out)))
        return out

    def trunk_stances_device(self, d_queries_ptr, n, d_out_ptr, limits=None, stream=0):
        """Device form: DEVICE pointers to n queries and n records, asynchronous on `stream`."""
        tl = _trunk_limits(limits)
        self._check(self._lib.fpe_trunk_stances_device(self._h, ptr(self.params), C.byref(tl) if tl is not None else None,
                                                       C.c_void_p(d_queries_ptr), int(n), C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)))

    def plan_trunk(self, poses, n_cycles, limits=None, strides=None, products=("nominal", "cycle_ok"), summary=True):
        """fpe_trunk_plan with host buffers: plans the batch as plan() does (strides: as there) and checks the body box of every
        planned stance against the elevation layer in the same call.  Returns the requested plan products plus "trunk":
        TRUNK_RECORD_DTYPE [B, n_cycles] and (summary=True) "trunk_summary": TRUNK_SUMMARY_DTYPE [B]."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        unknown = set(products) - set(PRODUCT_ORDER)
        if unknown:
            raise ValueError(f"unknown plan products {sorted(unknown)}")
        shapes = product_shapes(B, n_cycles)
        out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in PRODUCT_ORDER if k in products}
        po = _fill_products(PlanOut(), {k: ptr(out[k]) for k in out})
        out["trunk"] = np.zeros((B, n_cycles), _capi.TRUNK_RECORD_DTYPE)
        to = _capi.TrunkOut(ptr(out["trunk"]), None)
        if summary:
            out["trunk_summary"] = np.zeros(B, _capi.TRUNK_SUMMARY_DTYPE)
            to.summary = ptr(out["trunk_summary"])
        tl = _trunk_limits(limits)
        self._check(self._lib.fpe_trunk_plan(self._h, ptr(self.params), C.byref(tl) if tl is not None else None, ptr(poses),
                                             ptr(_strides_for(strides, B)) if strides is not None else None, B, int(n_cycles),
                                             C.byref(po), C.byref(to)))
        return out

    def trunk_plan_device(self, d_nominal_ptr, d_cycle_ok_ptr, B, n_cycles, d_records_ptr=0, d_summary_ptr=0, limits=None, stream=0):
        """fpe_trunk_plan_device: DEVICE pointers to a plan's nominal and cycle_ok products as a plan call on `stream` left them and
        the outputs (0 = not wanted)."""
        po = _fill_products(PlanOut(), {"nominal": d_nominal_ptr, "cycle_ok": d_cycle_ok_ptr})
        to = _capi.TrunkOut(d_records_ptr or None, d_summary_ptr or None)
        tl = _trunk_limits(limits)
        self._check(self._lib.fpe_trunk_plan_device(self._h, ptr(self.params), C.byref(tl) if tl is not None else None, C.byref(po),
                                                    int(B), int(n_cycles), C.byref(to), C.c_void_p(stream or 0)))

    # ---- edge margin: distance from cells and planned footholds to bad ground (build-defined: fpe_margin_*) ---------------
    def margin_map(self, mp=None, roi=None, products=("dist_sq", "nearest")):
        """fpe_margin_map on the current map: {"dist_sq": uint16 [n_rows, n_cols] (MARGIN_NONE: no bad cell within reach), "nearest":
        int8 [n_rows, n_cols, 2] (di, dj)} for the requested products.  `mp`: None (classes candidate | unknown | off-map, reach 8, no
        limit), make_margin_params(...) or a dict of its keywords; roi as in foothold_map."""
        r, out, mo = self._dense_outputs("margin-map", roi, products)
        m = _margin_params(mp)
        self._check(self._lib.fpe_margin_map(self._h, ptr(self.params), C.byref(m) if m is not None else None, ptr(r), C.byref(mo)))
        return out

    def margin_map_device(self, d_dist_sq_ptr, d_nearest_ptr, mp=None, roi=None, stream=0):
        """Device form: DEVICE pointers (0 = product not wanted), asynchronous on `stream`."""
        r = self._roi(roi)
        mo = self._dense_out("margin-map", dist_sq=d_dist_sq_ptr, nearest=d_nearest_ptr)
        m = _margin_params(mp)
        self._check(self._lib.fpe_margin_map_device(self._h, ptr(self.params), C.byref(m) if m is not None else None, ptr(r), C.byref(mo),
                                                    C.c_void_p(stream or 0)))

    def margin_cells(self, cells, mp=None):
        """fpe_margin_cells: one MARGIN_RECORD_DTYPE record per cell of `cells` ([n, 2] canonical (row, col), in the map or not, or a
        MARGIN_QUERY_DTYPE array) on the current map."""
        if not (isinstance(cells, np.ndarray) and cells.dtype == _capi.MARGIN_QUERY_DTYPE):
            rc = np.asarray(cells, dtype=np.int32).reshape(-1, 2)
            cells = np.zeros(rc.shape[0], dtype=_capi.MARGIN_QUERY_DTYPE)
            cells["row"], cells["col"] = rc[:, 0], rc[:, 1]
        queries = np.ascontiguousarray(cells).reshape(-1)
        out = np.zeros(queries.shape[0], dtype=_capi.MARGIN_RECORD_DTYPE)
        m = _margin_params(mp)
        self._check(self._lib.fpe_margin_cells(self._h, ptr(self.params), C.byref(m) if m is not None else None, ptr(queries),
                                               queries.shape[0], ptr(out)))
        return out

    def margin_cells_device(self, d_queries_ptr, n, d_out_ptr, mp=None, stream=0):
        """Device form: DEVICE pointers to n queries and n records, asynchronous on `stream`."""
        m = _margin_params(mp)
        self._check(self._lib.fpe_margin_cells_device(self._h, ptr(self.params), C.byref(m) if m is not None else None,
                                                      C.c_void_p(d_queries_ptr), int(n), C.c_void_p(d_out_ptr), C.c_void_p(stream or 0)))

    def margin_plan(self, poses, n_cycles, mp=None, strides=None, products=("nominal",), summary=True):
        """fpe_margin_plan with host buffers: plans the batch as plan() does (strides: as there) and measures the margin of every
        planned foothold's cell in the same call.  Returns the requested plan products plus "margin": MARGIN_RECORD_DTYPE
        [B, n_cycles, 4] and (summary=True) "margin_summary": MARGIN_SUMMARY_DTYPE [B]."""
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        unknown = set(products) - set(PRODUCT_ORDER)
        if unknown:
            raise ValueError(f"unknown plan products {sorted(unknown)}")
        shapes = product_shapes(B, n_cycles)
        out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in PRODUCT_ORDER if k in products}
        po = _fill_products(PlanOut(), {k: ptr(out[k]) for k in out})
        out["margin"] = np.zeros((B, n_cycles, 4), _capi.MARGIN_RECORD_DTYPE)
        mo = _capi.MarginOut(ptr(out["margin"]), None)
        if summary:
            out["margin_summary"] = np.zeros(B, _capi.MARGIN_SUMMARY_DTYPE)
            mo.summary = ptr(out["margin_summary"])
        m = _margin_params(mp)
        self._check(self._lib.fpe_margin_plan(self._h, ptr(self.params), C.byref(m) if m is not None else None, ptr(poses),
                                              ptr(_strides_for(strides, B)) if strides is not None else None, B, int(n_cycles),
                                              C.byref(po), C.byref(mo)))
        return out

    def margin_plan_device(self, d_nominal_ptr, B, n_cycles, d_records_ptr=0, d_summary_ptr=0, mp=None, stream=0):
        """fpe_margin_plan_device: a DEVICE pointer to a plan's nominal product as a plan call on `stream` left it, and the outputs
        (0 = not wanted)."""
        po = _fill_products(PlanOut(), {"nominal": d_nominal_ptr})
        mo = _capi.MarginOut(d_records_ptr or None, d_summary_ptr or None)
        m = _margin_params(mp)
        self._check(self._lib.fpe_margin_plan_device(self._h, ptr(self.params), C.byref(m) if m is not None else None, C.byref(po),
                                                     int(B), int(n_cycles), C.byref(mo), C.c_void_p(stream or 0)))

    # ---- the dense maps as grid_map message layers (fpe_export_layers*) ----------------------------------------------------
    def _layer_request(self, names, dsts, snap_search_radius, snap_polygon, centroid_search_radius):
        """fpe_layer_request for layer names and their destinations (addresses); unknown names raise before the library is called."""
        names = list(names)
        unknown = [n for n in names if n not in _capi.LAYER_NAMES]
        if unknown:
            raise ValueError(f"unknown layers {sorted(unknown)}")
        if len(names) > _capi.LAYER_COUNT:
            raise ValueError(f"at most {_capi.LAYER_COUNT} layers, each once")
        rq = _capi.LayerRequest()
        rq.n_layers = len(names)
        for k, (n, d) in enumerate(zip(names, dsts)):
            rq.layer[k] = _capi.LAYER_NAMES.index(n)
            rq.dst[k] = d
        rq.snap_search_radius = float(snap_search_radius or 0.0)
        rq.snap_polygon_kind = self._polygon_kind(snap_polygon)
        rq.centroid_search_radius = float(centroid_search_radius or 0.0)
        return rq

    @staticmethod
    def _layer_layout(start_index, storage_order):
        if storage_order not in ("col", "row"):
            raise ValueError(f"unknown storage order {storage_order!r}")
        return _capi.LayerLayout((C.c_int32 * 2)(*map(int, start_index)), 1 if storage_order == "row" else 0, 0)

    def export_layers(self, layers=_capi.LAYER_NAMES, roi=None, start_index=(0, 0), storage_order="col", snap_search_radius=None,
                      snap_polygon="rectangle", centroid_search_radius=None, pinned=False, out=None):
        """fpe_export_layers on the current map: {name: float32 array of the WHOLE map} for the requested layers
        (_capi.LAYER_NAMES), in the layout of the message being filled — shape (cols, rows) for storage_order "col" (the
        grid_map_msgs column-major buffer), (rows, cols) for "row", rotated by `start_index`, NaN outside `roi` — which is what
        gridmapCallback accepts with the same start_index and storage_order.  pinned: the arrays come from host_array (written by
        DMA, alive until close()); out: {name: C-contiguous float32 array of that shape} to fill instead of fresh arrays."""
        layers = list(layers)
        unknown = [n for n in layers if n not in _capi.LAYER_NAMES]
        if unknown:
            raise ValueError(f"unknown layers {sorted(unknown)}")
        lay = self._layer_layout(start_index, storage_order)
        info = self.map_info()
        shape = (info["rows"], info["cols"]) if storage_order == "row" else (info["cols"], info["rows"])
        if out is None:
            out = {n: (self.host_array(shape, np.float32) if pinned else np.empty(shape, np.float32)) for n in layers}
        for n in layers:
            a = out[n]
            if a.dtype != np.float32 or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError(f"layer {n!r}: the destination must be a C-contiguous float32 array of shape {shape}")
        rq = self._layer_request(layers, [out[n].ctypes.data for n in layers], snap_search_radius, snap_polygon, centroid_search_radius)
        self._check(self._lib.fpe_export_layers(self._h, ptr(self.params), ptr(self._roi(roi)), C.byref(lay), C.byref(rq)))
        return {n: out[n] for n in layers}

    def export_layers_device(self, d_layer_ptrs, roi=None, start_index=(0, 0), storage_order="col", snap_search_radius=None,
                             snap_polygon="rectangle", centroid_search_radius=None, stream=0):
        """Device form: d_layer_ptrs = {name: DEVICE pointer to rows * cols floats}, asynchronous on `stream`."""
        names = list(d_layer_ptrs)
        rq = self._layer_request(names, [int(d_layer_ptrs[n]) for n in names], snap_search_radius, snap_polygon, centroid_search_radius)
        lay = self._layer_layout(start_index, storage_order)
        self._check(self._lib.fpe_export_layers_device(self._h, ptr(self.params), ptr(self._roi(roi)), C.byref(lay), C.byref(rq),
                                                       C.c_void_p(stream or 0)))

    # ---- the service (globalFootholdPlan, cpp:539-1602): response content for one pose ---------------------
    @staticmethod
    def _msg(m):
        n = int(m["n_footholds"])
        return {
            "success": bool(m["success"]),
            "gait_cycles": int(m["gait_cycles"]),
            "gait_cycles_succeed": int(m["gait_cycles_succeed"]),
            "footholds": m["footholds"][:n].copy(),
        }

    def last_service_gate(self):
        """fpe_last_service_gate: verdict of the handler's gate for this thread's last globalFootholdPlan call."""
        g = _capi.ServiceGate()
        self._check(self._lib.fpe_last_service_gate(self._h, C.byref(g)))
        return {"fail_cycle": int(g.fail_cycle), "fail_kind": int(g.fail_kind), "chain_ran": bool(g.chain_ran),
                "returned_false": bool(g.returned_false), "lf_current_row": float(g.lf_current_row), "rh_current_row": float(g.rh_current_row)}

    @staticmethod
    def _report(r):
        return {"path": r["feet_center_path"][: int(r["n_path"])].copy(),
                "feet_distance": r["feet_distance"][: int(r["n_kpi"])].copy(),
                "cog_speed": r["cog_speed"][: int(r["n_kpi"])].copy()}

    def globalFootholdPlan(self, gait_cycles, initial_position, all_tracks=False):
        """Response content of the service, or False where the reference's handler returns false
        (getGaitCycleSearchGridMap fails, cpp:920-934: in the first gait cycle, or on its lateral side in any cycle — the x side of
        later cycles follows the build-defined optimiser and refuses under set_tuning(service_opt_gate=2), the default; last_service_gate()
        tells the kinds apart); with all_tracks also the centroid message, the default-track
        rows (global_footholds_centroid, globalFootholdsResult_.defaultFootholds), and per track the
        feet-centre path and KPIs (nominal/centroid_feet_center_path, footholdsKPI_)."""
        if not all_tracks:
            # the latency path: message and position buffers of the planner's own, their addresses and the parameter block's taken once
            # (numpy's .ctypes and a zeroed 5 KB message per call were ~4 us of a 105 us call); the library fills every field it reports
            tls = self.__dict__.get("_svc_tls")
            if tls is None:
                tls = self.__dict__.setdefault("_svc_tls", threading.local())
            sv = getattr(tls, "sv", None)  # (per thread: the engine serves concurrent callers of one handle)
            if sv is None or sv[4] is not self.params:
                m, q = np.zeros(1, dtype=GLOBAL_FOOTHOLDS_DTYPE), np.zeros(3, dtype=np.float64)
                sv = tls.sv = (m, q, ptr(m), ptr(q), self.params, ptr(self.params),
                               m["success"], m["gait_cycles"], m["gait_cycles_succeed"], m["n_footholds"], m["footholds"][0])  # field views, made once
            sv[1][:] = np.asarray(initial_position, np.float64).reshape(3)  # (as the all_tracks path: three values or a ValueError, never a broadcast)
            rc = self._lib.fpe_plan_service(self._h, sv[5], sv[3], int(gait_cycles) & 0xFF, sv[2])
            if rc == _capi.FPE_E_SERVICE_FALSE:
                return False  # the reference's handler returns false here (cpp:931-934): the ROS call fails
            if rc != _capi.FPE_OK:
                self._check(rc)
            return {"success": bool(sv[6][0]), "gait_cycles": int(sv[7][0]), "gait_cycles_succeed": int(sv[8][0]),
                    "footholds": sv[10][: int(sv[9][0])].copy()}  # (= self._msg(sv[0][0]))
        msg = np.zeros(1, dtype=GLOBAL_FOOTHOLDS_DTYPE)
        pos = np.ascontiguousarray(initial_position, dtype=np.float64).reshape(3)
        cen = np.zeros(1, dtype=GLOBAL_FOOTHOLDS_DTYPE)
        optm = np.zeros(1, dtype=GLOBAL_FOOTHOLDS_DTYPE)
        dflt = np.zeros((1 + int(gait_cycles), 4, 3), dtype=np.float64)
        nrows = C.c_int32(0)
        rep = np.zeros(3, dtype=TRACK_REPORT_DTYPE)
        cyc = np.zeros(max(int(gait_cycles), 1), dtype=OPT_CYCLE_DTYPE)
        rc = self._lib.fpe_plan_service_opt(self._h, ptr(self.params), ptr(self.opt_params), ptr(pos), int(gait_cycles) & 0xFF,
                                            ptr(msg), ptr(cen), ptr(dflt), C.cast(C.byref(nrows), C.c_void_p), ptr(rep[0:1]),
                                            ptr(rep[1:2]), ptr(optm), ptr(rep[2:3]), ptr(cyc))
        if rc == _capi.FPE_E_SERVICE_FALSE:
            return False
        self._check(rc)
        out = self._msg(msg[0])
        out["centroid"] = self._msg(cen[0])
        out["default_footholds"] = dflt[: nrows.value].copy()
        out["report"] = self._report(rep[0])
        out["centroid"]["report"] = self._report(rep[1])
        out["opt"] = self._msg(optm[0])  # global_footholds_opt (cpp:221, 1510-1532)
        out["opt"]["report"] = self._report(rep[2])
        out["opt"]["cycles"] = cyc[: int(gait_cycles)].copy()
        return out


class ScanState:
    """A scan state of one engine (fpe_scan_*; include/fpe.h): a robot-centric elevation layer and its variance layer in HBM, into
    which point clouds are fused.  Made by FootholdPlanner.scan_state(); close it before its planner.  The device forms take device
    addresses and a stream handle and never synchronise the host."""

    def __init__(self, planner, rows, cols, resolution, position=(0.0, 0.0)):
        self._planner, self._lib = planner, planner._lib
        self._s = C.c_void_p()
        d = _map_desc(rows, cols, resolution, position)
        planner._check(self._lib.fpe_scan_create(planner._h, C.byref(d), C.byref(self._s)))
        self.rows, self.cols, self.resolution = int(rows), int(cols), float(resolution)

    def close(self):
        if getattr(self, "_s", None) and getattr(self._planner, "_h", None):
            self._lib.fpe_scan_destroy(self._s)
        self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        self._planner._check(rc)

    def geometry(self):
        d = MapDesc()
        self._check(self._lib.fpe_scan_geometry(self._s, C.byref(d)))
        return {"rows": d.rows, "cols": d.cols, "resolution": d.resolution, "position": tuple(d.position)}

    def set_layers(self, elevation, variance):
        """Both layers from (rows, cols) host arrays; a cell that is NaN in either becomes unknown in both.  Synchronous."""
        e, v = (np.ascontiguousarray(a, dtype=np.float32) for a in (elevation, variance))
        if e.shape != (self.rows, self.cols) or v.shape != e.shape:
            raise ValueError("set_layers takes two (rows, cols) arrays")
        self._check(self._lib.fpe_scan_set_layers(self._s, ptr(e), ptr(v)))

    def set_layers_device(self, d_elev_ptr, d_var_ptr, stream=None):
        self._check(self._lib.fpe_scan_set_layers_device(self._s, C.c_void_p(d_elev_ptr), C.c_void_p(d_var_ptr), C.c_void_p(stream or 0)))

    def read_layers(self, elevation=True, variance=True):
        """-> (elevation, variance) as (rows, cols) arrays, bit for bit (None for a layer not asked for).  Synchronous."""
        e = np.empty((self.rows, self.cols), np.float32) if elevation else None
        v = np.empty((self.rows, self.cols), np.float32) if variance else None
        self._check(self._lib.fpe_scan_read_layers(self._s, ptr(e), ptr(v)))
        return e, v

    def read_layers_device(self, d_elev_ptr=0, d_var_ptr=0, stream=None):
        self._check(self._lib.fpe_scan_read_layers_device(self._s, C.c_void_p(d_elev_ptr or 0), C.c_void_p(d_var_ptr or 0), C.c_void_p(stream or 0)))

    def move(self, shift, position, stream=None):
        """fpe_scan_move: new cell (i, j) takes old cell (i + sr, j + sc) of both layers, or becomes unknown; asynchronous."""
        sh, pos = (C.c_int32 * 2)(int(shift[0]), int(shift[1])), (C.c_double * 2)(float(position[0]), float(position[1]))
        self._check(self._lib.fpe_scan_move(self._s, sh, pos, C.c_void_p(stream or 0)))

    @staticmethod
    def _points(points, scan):
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.size < scan.n_points * scan.point_stride:
            raise ValueError("fewer floats than n_points * point_stride")
        return p if p.size else np.zeros(3, np.float32)  # (n_points == 0: any non-null address)

    def fuse(self, scan, points, params=None):
        """fpe_scan_fuse: host points ((n, point_stride) floats) -> the call's info as a SCAN_INFO_DTYPE record.  Synchronous."""
        p = self._points(points, scan)
        info = np.zeros(1, _capi.SCAN_INFO_DTYPE)
        self._check(self._lib.fpe_scan_fuse(self._s, C.byref(params if params is not None else scan_params()), C.byref(scan), ptr(p), ptr(info)))
        return info[0]

    def fuse_device(self, scan, d_points_ptr, params=None, d_info_ptr=0, stream=None):
        """fpe_scan_fuse_device: device points, a device info of sixteen int32 (0: not wanted); asynchronous on `stream`."""
        self._check(self._lib.fpe_scan_fuse_device(self._s, C.byref(params if params is not None else scan_params()), C.byref(scan),
                                                   C.c_void_p(d_points_ptr), C.c_void_p(d_info_ptr or 0), C.c_void_p(stream or 0)))

    def install(self, filter_params=None, stream=None):
        """fpe_scan_install: the state's content becomes the planner's current snapshot (filters, then an upload); asynchronous."""
        pl = self._planner
        self._check(self._lib.fpe_scan_install(pl._h, self._s, C.byref(filter_params) if filter_params is not None else None, C.c_void_p(stream or 0)))
        pl.rows, pl.cols, pl.resolution = self.rows, self.cols, self.resolution

    @staticmethod
    def _move_args(shift, position):
        return (C.c_int32 * 2)(int(shift[0]), int(shift[1])), (C.c_double * 2)(float(position[0]), float(position[1]))

    def ingest(self, scan, points, shift, position, params=None, filter_params=None):
        """fpe_scan_ingest: move (when the shift or the position says so), fuse, and the roi into the snapshot through an
        elevation-driven update -> (scan info record, update info dict).  Synchronous."""
        p = self._points(points, scan)
        sh, pos = self._move_args(shift, position)
        info, ui = np.zeros(1, _capi.SCAN_INFO_DTYPE), _capi.ElevationUpdateInfo()
        self._check(self._lib.fpe_scan_ingest(self._planner._h, self._s, C.byref(filter_params) if filter_params is not None else None,
                                              C.byref(params if params is not None else scan_params()), C.byref(scan), ptr(p), sh, pos, ptr(info),
                                              C.byref(ui)))
        return info[0], _info_dict(ui)

    def ingest_device(self, scan, d_points_ptr, shift, position, params=None, filter_params=None, d_info_ptr=0, stream=None):
        """fpe_scan_ingest_device: the same with device points and a device scan info (0: not wanted), asynchronous on `stream` ->
        the update info dict."""
        sh, pos = self._move_args(shift, position)
        ui = _capi.ElevationUpdateInfo()
        self._check(self._lib.fpe_scan_ingest_device(self._planner._h, self._s, C.byref(filter_params) if filter_params is not None else None,
                                                     C.byref(params if params is not None else scan_params()), C.byref(scan),
                                                     C.c_void_p(d_points_ptr), sh, pos, C.c_void_p(d_info_ptr or 0), C.byref(ui),
                                                     C.c_void_p(stream or 0)))
        return _info_dict(ui)

    # ---- visibility clearing: cells a scan sees through become unknown (fpe_scan_clear*) -------------------------------
    def clear(self, scan, points, params=None, clear_params=None):
        """fpe_scan_clear: host points -> the call's info as a SCAN_CLEAR_INFO_DTYPE record.  Synchronous."""
        p = self._points(points, scan)
        info = np.zeros(1, _capi.SCAN_CLEAR_INFO_DTYPE)
        self._check(self._lib.fpe_scan_clear(self._s, C.byref(params if params is not None else scan_params()),
                                             C.byref(clear_params if clear_params is not None else scan_clear_params()), C.byref(scan), ptr(p), ptr(info)))
        return info[0]

    def clear_device(self, scan, d_points_ptr, params=None, clear_params=None, d_info_ptr=0, stream=None):
        """fpe_scan_clear_device: device points, a device info of 64 bytes (0: not wanted); asynchronous on `stream`."""
        self._check(self._lib.fpe_scan_clear_device(self._s, C.byref(params if params is not None else scan_params()),
                                                    C.byref(clear_params if clear_params is not None else scan_clear_params()), C.byref(scan),
                                                    C.c_void_p(d_points_ptr), C.c_void_p(d_info_ptr or 0), C.c_void_p(stream or 0)))

    def ingest_clear(self, scan, points, shift, position, params=None, clear_params=None, filter_params=None):
        """fpe_scan_ingest_clear: move (when the shift or the position says so), clear, fuse, and the roi into the snapshot ->
        (clear info record, scan info record, update info dict).  Synchronous."""
        p = self._points(points, scan)
        sh, pos = self._move_args(shift, position)
        cinfo, info, ui = np.zeros(1, _capi.SCAN_CLEAR_INFO_DTYPE), np.zeros(1, _capi.SCAN_INFO_DTYPE), _capi.ElevationUpdateInfo()
        self._check(self._lib.fpe_scan_ingest_clear(self._planner._h, self._s, C.byref(filter_params) if filter_params is not None else None,
                                                    C.byref(params if params is not None else scan_params()),
                                                    C.byref(clear_params if clear_params is not None else scan_clear_params()), C.byref(scan), ptr(p),
                                                    sh, pos, ptr(cinfo), ptr(info), C.byref(ui)))
        return cinfo[0], info[0], _info_dict(ui)

    def ingest_clear_device(self, scan, d_points_ptr, shift, position, params=None, clear_params=None, filter_params=None, d_clear_info_ptr=0,
                            d_info_ptr=0, stream=None):
        """fpe_scan_ingest_clear_device: the same with device points and device infos (0: not wanted), asynchronous on `stream` ->
        the update info dict."""
        sh, pos = self._move_args(shift, position)
        ui = _capi.ElevationUpdateInfo()
        self._check(self._lib.fpe_scan_ingest_clear_device(self._planner._h, self._s, C.byref(filter_params) if filter_params is not None else None,
                                                           C.byref(params if params is not None else scan_params()),
                                                           C.byref(clear_params if clear_params is not None else scan_clear_params()), C.byref(scan),
                                                           C.c_void_p(d_points_ptr), sh, pos, C.c_void_p(d_clear_info_ptr or 0),
                                                           C.c_void_p(d_info_ptr or 0), C.byref(ui), C.c_void_p(stream or 0)))
        return _info_dict(ui)

    # ---- gap closing: small holes of the elevation bridged for the planner (fpe_scan_close*) ---------------------------
    # (`close()` is the state's destructor, so the binding of fpe_scan_close is called close_gaps)
    def close_gaps(self, rect=None, close_params=None, classes=True, row_stride=None):
        """fpe_scan_close: the closed elevation of `rect` = (row0, col0, n_rows, n_cols) (None: the whole state) -> ((n_rows,
        n_cols) float32 array, uint8 class array or None, SCAN_CLOSE_INFO_DTYPE record).  The state is not written.  Synchronous.
        row_stride: the pitch of the buffers the call writes (the arrays returned are views of their first n_cols columns)."""
        r = (0, 0, self.rows, self.cols) if rect is None else tuple(int(x) for x in rect)
        pitch = int(row_stride) if row_stride is not None else max(r[3], 1)
        out = np.zeros((max(r[2], 1), max(pitch, 1)), np.float32)
        cls = np.zeros(out.shape, np.uint8) if classes else None
        info = np.zeros(1, _capi.SCAN_CLOSE_INFO_DTYPE)
        self._check(self._lib.fpe_scan_close(self._s, C.byref(close_params if close_params is not None else scan_close_params()), _rect(r), ptr(out),
                                             pitch, ptr(cls), ptr(info)))
        return out[:r[2], :r[3]], (cls[:r[2], :r[3]] if classes else None), info[0]

    def close_gaps_device(self, rect, d_out_ptr, row_stride, close_params=None, d_cls_ptr=0, d_info_ptr=0, stream=None):
        """fpe_scan_close_device: device buffers with a pitch of `row_stride` elements, a device info of 64 bytes (0: not wanted);
        asynchronous on `stream`."""
        self._check(self._lib.fpe_scan_close_device(self._s, C.byref(close_params if close_params is not None else scan_close_params()), _rect(rect),
                                                    C.c_void_p(d_out_ptr), int(row_stride), C.c_void_p(d_cls_ptr or 0), C.c_void_p(d_info_ptr or 0),
                                                    C.c_void_p(stream or 0)))

    def install_closed(self, close_params=None, filter_params=None, stream=None):
        """fpe_scan_install_closed: install with the closed whole-map layer in place of the state's elevation; asynchronous."""
        pl = self._planner
        self._check(self._lib.fpe_scan_install_closed(pl._h, self._s, C.byref(filter_params) if filter_params is not None else None,
                                                      C.byref(close_params if close_params is not None else scan_close_params()), C.c_void_p(stream or 0)))
        pl.rows, pl.cols, pl.resolution = self.rows, self.cols, self.resolution

    def ingest_closed(self, scan, points, shift, position, params=None, clear_params=None, close_params=None, filter_params=None):
        """fpe_scan_ingest_closed: move, the clear (when clear_params is given), fuse, the close of the touched rectangles, and those
        into the snapshot -> (clear info record or None, scan info record, close info record, update info dict).  Synchronous."""
        p = self._points(points, scan)
        sh, pos = self._move_args(shift, position)
        cinfo, info, kinfo = np.zeros(1, _capi.SCAN_CLEAR_INFO_DTYPE), np.zeros(1, _capi.SCAN_INFO_DTYPE), np.zeros(1, _capi.SCAN_CLOSE_INFO_DTYPE)
        ui = _capi.ElevationUpdateInfo()
        self._check(self._lib.fpe_scan_ingest_closed(self._planner._h, self._s, C.byref(filter_params) if filter_params is not None else None,
                                                     C.byref(params if params is not None else scan_params()),
                                                     C.byref(clear_params) if clear_params is not None else None,
                                                     C.byref(close_params if close_params is not None else scan_close_params()), C.byref(scan), ptr(p),
                                                     sh, pos, ptr(cinfo), ptr(info), ptr(kinfo), C.byref(ui)))
        return (cinfo[0] if clear_params is not None else None), info[0], kinfo[0], _info_dict(ui)

    def ingest_closed_device(self, scan, d_points_ptr, shift, position, params=None, clear_params=None, close_params=None, filter_params=None,
                             d_clear_info_ptr=0, d_info_ptr=0, d_close_info_ptr=0, stream=None):
        """fpe_scan_ingest_closed_device: the same with device points and device infos (0: not wanted), asynchronous on `stream` ->
        the update info dict."""
        sh, pos = self._move_args(shift, position)
        ui = _capi.ElevationUpdateInfo()
        self._check(self._lib.fpe_scan_ingest_closed_device(self._planner._h, self._s, C.byref(filter_params) if filter_params is not None else None,
                                                            C.byref(params if params is not None else scan_params()),
                                                            C.byref(clear_params) if clear_params is not None else None,
                                                            C.byref(close_params if close_params is not None else scan_close_params()), C.byref(scan),
                                                            C.c_void_p(d_points_ptr), sh, pos, C.c_void_p(d_clear_info_ptr or 0),
                                                            C.c_void_p(d_info_ptr or 0), C.c_void_p(d_close_info_ptr or 0), C.byref(ui),
                                                            C.c_void_p(stream or 0)))
        return _info_dict(ui)

    # ---- scan images: a depth or range image as the point source, without a point cloud (fpe_scan_*_image*) --------------
    # `scan.n_points` is the number of selected pixels (scan_image_selected); `im` comes from make_scan_image.
    image_points = staticmethod(scan_image_points)

    def fuse_image(self, scan, im, image, params=None):
        """fpe_scan_fuse_image: a host image (and host tables) -> the call's info as a SCAN_INFO_DTYPE record.  Synchronous."""
        a = _image(image, im)
        info = np.zeros(1, _capi.SCAN_INFO_DTYPE)
        self._check(self._lib.fpe_scan_fuse_image(self._s, C.byref(params if params is not None else scan_params()), C.byref(scan), C.byref(im), ptr(a),
                                                  ptr(info)))
        return info[0]

    def fuse_image_device(self, scan, im, d_image_ptr, params=None, d_info_ptr=0, stream=None):
        """fpe_scan_fuse_image_device: a device image (the descriptor's tables are device addresses), a device info of sixteen int32
        (0: not wanted); asynchronous on `stream`."""
        self._check(self._lib.fpe_scan_fuse_image_device(self._s, C.byref(params if params is not None else scan_params()), C.byref(scan), C.byref(im),
                                                         C.c_void_p(d_image_ptr), C.c_void_p(d_info_ptr or 0), C.c_void_p(stream or 0)))

    def clear_image(self, scan, im, image, params=None, clear_params=None):
        """fpe_scan_clear_image: a host image -> the call's info as a SCAN_CLEAR_INFO_DTYPE record.  Synchronous."""
        a = _image(image, im)
        info = np.zeros(1, _capi.SCAN_CLEAR_INFO_DTYPE)
        self._check(self._lib.fpe_scan_clear_image(self._s, C.byref(params if params is not None else scan_params()),
                                                   C.byref(clear_params if clear_params is not None else scan_clear_params()), C.byref(scan),
                                                   C.byref(im), ptr(a), ptr(info)))
        return info[0]

    def clear_image_device(self, scan, im, d_image_ptr, params=None, clear_params=None, d_info_ptr=0, stream=None):
        """fpe_scan_clear_image_device: a device image, a device info of 64 bytes (0: not wanted); asynchronous on `stream`."""
        self._check(self._lib.fpe_scan_clear_image_device(self._s, C.byref(params if params is not None else scan_params()),
                                                          C.byref(clear_params if clear_params is not None else scan_clear_params()), C.byref(scan),
                                                          C.byref(im), C.c_void_p(d_image_ptr), C.c_void_p(d_info_ptr or 0), C.c_void_p(stream or 0)))

    def ingest_image(self, scan, im, image, shift, position, params=None, clear_params=None, close_params=None, filter_params=None):
        """fpe_scan_ingest_image: ingest (neither clear_params nor close_params), ingest_clear (clear_params) or ingest_closed
        (close_params, with or without clear_params) of a host image -> (clear info record or None, scan info record, close info
        record or None, update info dict).  Synchronous."""
        a = _image(image, im)
        sh, pos = self._move_args(shift, position)
        cinfo, info, kinfo = np.zeros(1, _capi.SCAN_CLEAR_INFO_DTYPE), np.zeros(1, _capi.SCAN_INFO_DTYPE), np.zeros(1, _capi.SCAN_CLOSE_INFO_DTYPE)
        ui = _capi.ElevationUpdateInfo()
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
        self._check(self._lib.fpe_scan_ingest_image(self._planner._h, self._s, ref(filter_params), C.byref(params if params is not None else scan_params()),
                                                    ref(clear_params), ref(close_params), C.byref(scan), C.byref(im), ptr(a), sh, pos, ptr(cinfo),
                                                    ptr(info), ptr(kinfo), C.byref(ui)))
        return (cinfo[0] if clear_params is not None else None), info[0], (kinfo[0] if close_params is not None else None), _info_dict(ui)

    def ingest_image_device(self, scan, im, d_image_ptr, shift, position, params=None, clear_params=None, close_params=None, filter_params=None,
                            d_clear_info_ptr=0, d_info_ptr=0, d_close_info_ptr=0, stream=None):
        """fpe_scan_ingest_image_device: the same with a device image and device infos (0: not wanted), asynchronous on `stream` ->
        the update info dict."""
        sh, pos = self._move_args(shift, position)
        ui = _capi.ElevationUpdateInfo()
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
        self._check(self._lib.fpe_scan_ingest_image_device(self._planner._h, self._s, ref(filter_params),
                                                           C.byref(params if params is not None else scan_params()), ref(clear_params),
                                                           ref(close_params), C.byref(scan), C.byref(im), C.c_void_p(d_image_ptr), sh, pos,
                                                           C.c_void_p(d_clear_info_ptr or 0), C.c_void_p(d_info_ptr or 0),
                                                           C.c_void_p(d_close_info_ptr or 0), C.byref(ui), C.c_void_p(stream or 0)))
        return _info_dict(ui)


class MultiFootholdPlanner(_Handle):
    """Several GPUs in ONE process behind the C ABI (fpe_multi_*): the map is replicated on every device and a pose
    batch is split into contiguous blocks, one host thread per device (include/fpe.h, "several GPUs")."""
    _CREATE, _DESTROY, _LAST_ERROR = "fpe_multi_create", "fpe_multi_destroy", "fpe_multi_last_error"

    def __init__(self, device_ids, params=None):
        ids = np.ascontiguousarray(device_ids, dtype=np.int32)
        self._create(ptr(ids), ids.size, params=params)

    @property
    def device_count(self):
        return int(self._lib.fpe_multi_device_count(self._h))

    def set_tuning(self, **kw):
        for k, v in kw.items():
            self._check(self._lib.fpe_multi_set_tuning(self._h, k.encode(), int(v)))

    def gridmapCallback(self, traversability, elevation, resolution, position=(0.0, 0.0)):
        trav = np.ascontiguousarray(traversability, dtype=np.float32)
        elev = np.ascontiguousarray(elevation, dtype=np.float32)
        rows, cols = trav.shape
        d = _map_desc(rows, cols, resolution, position)
        self._check(self._lib.fpe_multi_upload_map(self._h, C.byref(d), ptr(trav), ptr(elev)))

    def update_map(self, shift, position, patches=()):
        """fpe_multi_update_map: FootholdPlanner.update_map on every engine of the group."""
        raw, keep = _host_patches(patches)
        u = make_map_update(shift, position, raw)
        self._check(self._lib.fpe_multi_update_map(self._h, C.byref(u)))
        del keep

    def engine(self, k):
        return self._lib.fpe_multi_engine(self._h, int(k))

    def shard_range(self, B, k):
        first, count = C.c_int32(0), C.c_int32(0)
        rc = self._lib.fpe_multi_shard_range(int(B), int(k), self.device_count, C.byref(first), C.byref(count))
        if rc != _capi.FPE_OK:
            raise FpeError(rc, "bad shard arguments")
        return first.value, first.value + count.value

    def stream(self, k):
        return self._lib.fpe_multi_stream(self._h, int(k))

    def synchronize(self):
        self._check(self._lib.fpe_multi_synchronize(self._h))

    def plan_device(self, B, n_cycles, ios, record_kind=_capi.EXCHANGE_SELECTED):
        """fpe_multi_plan_device.  `ios`: per device a dict {"d_poses": ptr, "d_gathered": ptr, "stream": ptr or 0, and any of the
        product names of PRODUCT_ORDER: ptr} of DEVICE pointers on that device."""
        arr = (_capi.MultiDeviceIO * len(ios))()
        for k, d in enumerate(ios):
            arr[k].d_poses = d["d_poses"]
            for name, field in PRODUCT_FIELDS.items():
                if d.get(name):
                    setattr(arr[k].d_out, field, d[name])
            arr[k].d_gathered = d.get("d_gathered") or None
            arr[k].stream = d.get("stream") or None
        self._check(self._lib.fpe_multi_plan_device(self._h, ptr(self.params), arr, int(B), int(n_cycles), int(record_kind)))

    def plan(self, poses, n_cycles):
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE)
        B = poses.shape[0]
        shapes = product_shapes(B, n_cycles)
        out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in DEFAULT_PRODUCTS}
        po = PlanOut(*(ptr(out[k]) for k in DEFAULT_PRODUCTS))  # (DEFAULT_PRODUCTS are the struct's leading fields, in its order)
        self._check(self._lib.fpe_multi_plan(self._h, ptr(self.params), ptr(poses), B, int(n_cycles), C.byref(po)))
        return out
