/*
 * fpe.h — C ABI of the MI355X foothold-search engine (libfpe.so).
 *
 * Drop-in boundary for ONE hot path of lukechencqu/quadrupedal_foothold_planner: the per-leg
 * foothold search and per-cycle recurrence inside the `plan_global_footholds` service.
 * File:line citations are relative to the reference checkout
 * (foothold_planner/src/FootholdPlanner.cpp = "cpp", include/foothold_planner/FootholdPlanner.hpp
 * = "hpp").  The reference has no FFI of its own; each entry point names the reference seam it
 * replaces and INTEGRATION.md shows the binding a maintainer adds to FootholdPlanner.cpp.
 *
 * Conventions: every function returns an int status (FPE_OK = 0, negative = error); nothing
 * throws, nothing prints.  Callers own every host buffer; the engine owns device memory.  Inputs
 * are read-only and may be freed on return (synchronous entry points) or once the given stream
 * has passed the call (…_device entry points).  the fpe_upload_map, fpe_plan and fpe_search_legs families
 * may be called concurrently from different threads: a plan uses the map snapshot that was
 * current when it entered (the reference instead races on gridmap_, cpp:506 vs cpp:818).
 */
#ifndef FPE_H
#define FPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fpe_engine* fpe_handle;

enum fpe_status {
    FPE_OK = 0,
    FPE_E_INVALID_ARG = -1, /* null pointer, non-positive size, non-finite pose, too many vertices … */
    FPE_E_NO_MAP = -2,      /* plan/search before any fpe_upload_map (reference: empty gridmap_) */
    FPE_E_HIP = -3,         /* a HIP runtime call failed; fpe_last_error() has the text */
    FPE_E_NO_DEVICE = -4,   /* no usable gfx950 device / HIP code object not loadable */
    FPE_E_UNSUPPORTED = -5, /* search radius / foot radius too large for the on-chip tile */
    FPE_E_NOMEM = -6,
    FPE_E_SERVICE_FALSE = -7 /* the reference's service handler returns false for this request:
                                getGaitCycleSearchGridMap's getSubmap failed (cpp:920-934, 2345-2349) — for a reason
                                that does not depend on the optimiser (fpe_service_gate; "service_opt_gate" 2 widens it) */
};

/* ROS parameters of the path, with the reference's member types (readParameters cpp:248-314;
 * hpp:609-619, hpp:657-697).  Floats stay floats: the reference promotes them to double at each
 * use and that decides chosen indices (e.g. ceil(double(0.1f)/0.02) = 6 rings, not 5). */
typedef struct fpe_params {
    float footRadius;                 /* cpp:255 */
    float defaultFootholdThreshold;   /* cpp:257 */
    float candidateFootholdThreshold; /* cpp:258 */
    float searchRadius;               /* cpp:261 */
    float stepLength;                 /* cpp:262 */
    float length, width, l1;          /* laikago_kinematics/{length,width,l1}, cpp:285-287 */
    float skew;                       /* laikago_kinematics/skewLength -> isos_.skew, cpp:290 */
    int32_t RF_FIRST;                 /* cpp:264 */
    double h;                         /* h_ (cpp:336), hard-coded 0.01 in the reference */
    double lateralDrift;              /* ajustedPose_[1] += -0.007 per cycle (cpp:1578) */
} fpe_params;

/* yaml values of foothold_planner/config/foothold_planner.yaml:10-64 */
int fpe_params_yaml(fpe_params* out);
/* code defaults of readParameters (cpp:255-290) */
int fpe_params_code_defaults(fpe_params* out);

/* One element of the batch axis.  position = initialPose_ (cpp:293-295).  The remaining fields are
 * build-defined extensions (not in the reference): zeros reproduce the reference exactly. */
typedef struct fpe_pose {
    double position[3];
    int32_t gait;                /* 0 = trot (reference), 1 = 4-phase walk (build-defined) */
    float leg_search_radius[4];  /* RF,RH,LH,LF; <= 0 -> fpe_params.searchRadius */
    int32_t leg_polygon_kind[4]; /* 0 = reference rectangle getSearchPolygon (cpp:2496-2517);
                                    1 = build-defined hexagon */
} fpe_pose;

/* Geometry + storage of the traversability map message handed to gridmapCallback (cpp:504-536).
 * storage_order 0 = the grid_map_msgs/GridMap Float32MultiArray / Eigen::MatrixXf layout
 * (column-major: buffer cell (i,j) at i + j*rows); 1 = row-major.  start_index is the circular
 * buffer origin GridMap::getStartIndex() (= msg.outer_start_index / inner_start_index mapped by
 * GridMapRosConverter).  The engine canonicalises to start index (0,0),
 * row-major, on the device. */
typedef struct fpe_map_desc {
    int32_t rows, cols;     /* getSize()(0), getSize()(1): rows span x, cols span y */
    double resolution;      /* getResolution() */
    double position[2];     /* getPosition() (map centre) */
    int32_t start_index[2]; /* getStartIndex() (row, col) */
    int32_t storage_order;  /* 0 column-major, 1 row-major */
} fpe_map_desc;

/* One nominal-track foothold = result of checkFoothold (cpp:2001-2036, hpp:94-100). */
typedef struct fpe_foothold {
    int32_t row, col; /* chosen grid index: spiral cell, or getIndex(centre) for a default hit; -1 none */
    double x, y;      /* footholdResult.point.x/y (cell centre, or the continuous centre) */
    float z;          /* getFootholdMeanHeight (returns float, cpp:2520); 0 when invalid */
    uint8_t valid;    /* footholdValidation (cpp:2013, 2023) */
    uint8_t source;   /* 0 default-disc hit, 1 spiral candidate, 2 none, 3 radius over the tile bound */
    uint8_t foot_id;  /* Foothold.msg foot_id: 0 RF, 1 RH, 2 LH, 3 LF (cpp:686-698) */
    uint8_t gait_cycle_id; /* Foothold.msg gait_cycle_id = gaitCycleIndex (cpp:1378) */
} fpe_foothold;

/* One centroid-track foothold = result of checkFootholdUseCentroidMethod (cpp:1605-1997). */
typedef struct fpe_centroid_foothold {
    double x, y;
    float z;
    int32_t row, col; /* getIndex(x,y) on the full map; -1 when the result was left untouched */
    uint8_t code;     /* 0 whole region valid, 1 case 1, 2/3 case 2 upper/lower, 4 case 3,
                         5 no case (result (0,0,0)), 6 getSubmap failed (result (0,0,0)) */
    uint8_t pad[3];
} fpe_centroid_foothold;

/* The exchange record of a selected (nominal) foothold, 16 bytes: the chosen grid index, the height
 * and the flag bytes of the nominal record; x / y stay with the rank that planned the pose.  This is what
 * the multi-GPU all-gather moves. */
typedef struct fpe_selected_foothold {
    int32_t row, col;
    float z;
    uint8_t valid, source, foot_id, gait_cycle_id;
} fpe_selected_foothold;

/* The same record in 8 bytes (build-defined; the exchange of a multi-GPU step moves HALF the bytes): one word holding
 * the grid index and the two flags, and the height.  foot_id / gait_cycle_id are positional (record (b, g, leg) sits at
 * ((b * n_cycles) + g) * 4 + leg on every rank).  An index is stored with a bias of FPE_PACKED_BIAS in 14 bits: a default
 * hit carries getIndex(centre) (cpp:2016), which lies up to a foot radius OUTSIDE the map for a centre just over its edge
 * (found by the random campaign: col -3 of a valid foothold), and -1 ("no foothold") needs no code of its own.  Maps of up
 * to FPE_PACKED_MAX_CELLS rows / columns (fpe_plan* fail with FPE_E_UNSUPPORTED when the product is requested on a larger map). */
typedef struct fpe_selected_packed {
    uint32_t cell; /* bits 0-13 row + 256, 14-27 col + 256, bit 28 valid, bits 29-30 source, bit 31 zero */
    float z;
} fpe_selected_packed;
#define FPE_PACKED_BIAS 256
#define FPE_PACKED_MAX_CELLS (16383 - 2 * FPE_PACKED_BIAS)
#define FPE_PACKED_ROW(c) ((int32_t)((c) & 0x3FFFu) - FPE_PACKED_BIAS)
#define FPE_PACKED_COL(c) ((int32_t)(((c) >> 14) & 0x3FFFu) - FPE_PACKED_BIAS)
#define FPE_PACKED_VALID(c) (((c) >> 28) & 1u)
#define FPE_PACKED_SOURCE(c) (((c) >> 29) & 3u)

/* fpe_plan_out.pose_status bits */
#define FPE_POSE_OPT_SUBMAP_FAILED 1u /* getGaitCycleSearchGridMap (cpp:2307-2349) fails in the FIRST gait cycle:
                                         getSubmap(next feet centre, isos_.length x isos_.width) — the reference's
                                         service handler returns false there (cpp:920-934).  This bit of the PLAN kernels
                                         covers cycle 0; later cycles follow the opt track's own feet: fpe_plan_opt*
                                         (fpe_opt_out.gate_fail_cycle; see fpe_service_gate for what the service calls do). */

/* Output buffers of a chained plan; any pointer may be NULL (that product is skipped).
 * Index convention: record (b, g, leg) at ((b * n_cycles) + g) * 4 + leg. */
typedef struct fpe_plan_out {
    fpe_foothold* nominal;           /* [B * n_cycles * 4] — what the service returns (cpp:1588) */
    fpe_centroid_foothold* centroid; /* [B * n_cycles * 4] — global_footholds_centroid (cpp:1448-1462) */
    double* default_next;            /* [B * n_cycles * 4 * 3] default track x,y,z (cpp:1344-1347) */
    uint8_t* cycle_ok;               /* [B * n_cycles] footholdValidation_ per cycle (cpp:1323) */
    double* stance;                  /* [B * 4 * 3] RF/RH/LH/LF_initialPosition_ (cpp:350-378) */
    fpe_selected_foothold* selected; /* [B * n_cycles * 4] 16-byte form of `nominal` (multi-GPU exchange record) */
    uint8_t* pose_status;            /* [B] FPE_POSE_* bits */
    fpe_selected_packed* selected_packed; /* [B * n_cycles * 4] 8-byte form of `selected` (halves the exchange) */
} fpe_plan_out;

/* ---- the "opt" track: cpp:54-148 objective + constraints, cpp:913-1319 per-cycle driver,
 * cpp:1485-1570 commit, cpp:2307-2408 getGaitCycleSearchGridMap, cpp:2557-2568 getMapIndex ---------------------------
 * Reproduced exactly (bit for bit against the oracle): the gait-cycle submap gaitMap_, the four next default
 * positions, nominalIndex, checkFootholdUseCentroidMethod ON gaitMap_ with traversableBeginRow / traversableEndRow,
 * centroidIndex, the integer bounds xBounds, t1..t4, the objective and the eight constraints, positions and heights
 * taken from gaitMap_ at the optimiser's (truncated) x, the commit rule, lfCurrentRow / rhCurrentRow.
 * BUILD-DEFINED: the optimiser.  The reference runs NLopt's LN_COBYLA (yaml:60); NLopt is absent from this image and
 * unpinned by the reference, and COBYLA's iterates are not reproducible.  In its place: exhaustive search of the same
 * objective under the same constraints (tolerance ctol) over the INTEGER points of the same box — the reference
 * truncates x to int before using it (cpp:1287-1312) — feasible points by objective, else the point of least
 * constraint violation; deterministic tie-breaks (oracle/fpo_opt.cpp::solveLattice states the rule).  Against scipy's
 * COBYLA driving the same literal chain (tests/golden/cobyla_vs_lattice.json, build container only): identical x in 29 %
 * of the cycles, median distance 2 rows + 1 column, the handler's gate verdict identical for 94.8 % of 1 280 poses — the
 * opt products are a PLAUSIBLE track, not the reference's, and the gate verdict built on them is right about 19 times in 20
 * against a different COBYLA (against NLopt's: unmeasurable here). */
typedef struct fpe_opt_params {
    double w1, w2, w3, w4, wr, wc;         /* nlopt/w1..wc, cpp:297-303 */
    int32_t use_inequality_constraints;    /* nlopt/useInequalityConstraits, cpp:306 (code default 0, yaml 1) */
    int32_t reserved;
    double ctol;                           /* cpp:34: 1e-2 */
    double hip_lower_scale, hip_upper_scale;   /* cpp:48: 0.9, 1.1 */
    double skew_lower_scale, skew_upper_scale; /* cpp:49: 0.8, 1.2 */
    double lf_current_row0, rh_current_row0;   /* file-scope lfCurrentRow / rhCurrentRow (cpp:36) at entry of the call:
                                                  0 at node start, afterwards whatever the previous call left — the
                                                  adapter carries fpe_opt_out.rows_after / fpe_service_gate.lf/rh_current_row */
} fpe_opt_params;
int fpe_opt_params_yaml(fpe_opt_params* out);          /* yaml:53-63 + cpp:28-51 */
int fpe_opt_params_code_defaults(fpe_opt_params* out); /* cpp:297-307 (constraints off) */

/* RF/RH/LH/LF_footholdResult_opt of one cycle (cpp:1283-1314): record (b, g, leg) at ((b * n_cycles) + g) * 4 + leg. */
typedef struct fpe_opt_foothold {
    double x, y;      /* gaitMap_.getPosition((int)x[2k], (int)x[2k+1]) */
    float z;          /* getFootholdMeanHeight ON gaitMap_ (cpp:1290) */
    int32_t row, col; /* the truncated optimiser variables: an index of gaitMap_ */
    uint8_t foot_id, gait_cycle_id;
    uint8_t committed; /* the cycle committed (cpp:1332): the record is part of global_footholds_opt (cpp:1515-1532) */
    uint8_t pad;
} fpe_opt_foothold;

/* The optimisation problem of one gait cycle of one pose and its solution: record (b, g) at b * n_cycles + g.
 * Index order of the 8-vectors: LF, RH, RF, LH x (row, col) — the reference's x (cpp:50-51, 1058-1059). */
typedef struct fpe_opt_cycle {
    int32_t gait_top_left[2], gait_size[2]; /* gaitMap_ (cpp:2345) inside gridmap_: index of its cell (0,0); rows, cols */
    int32_t nominal_index[8];               /* cpp:965-976 */
    int32_t centroid_index[8];              /* cpp:1030-1041 */
    int32_t traversable_row[2][4];          /* cpp:1009-1013 / cpp:1608-1609: begin, end row x RF,RH,LH,LF (rows of gaitMap_);
                                               0 where the reference leaves its (uninitialised) storage untouched */
    int32_t x_lower[8], x_upper[8];         /* xBounds, cpp:1057-1076 */
    int32_t x[8];                           /* the optimiser's x as the reference uses it: truncated to int */
    double minf;                            /* objective at x */
    double lf_current_row, rh_current_row;  /* the values this cycle's objective and constraints 7-8 used */
    uint8_t centroid_code[4];               /* checkFootholdUseCentroidMethod on gaitMap_, RF,RH,LH,LF (fpe_centroid_foothold.code) */
    uint8_t gate_failed;                    /* getGaitCycleSearchGridMap returned false in THIS cycle (cpp:931-934) */
    uint8_t committed;
    uint8_t solver_status;                  /* 0 feasible optimum; 1 NLopt precondition (lb > ub or x0 outside the box: the
                                               reference's call throws, x stays x0); 2 least-violation point of an
                                               infeasible problem; 3 box too large to enumerate (x0 kept) */
    uint8_t pad;
} fpe_opt_cycle;

/* Outputs of the opt track; any pointer may be NULL.  Cycles from a pose's failing gate on (and every cycle of a
 * walk-gait pose: the opt track is the reference's, i.e. trot only) are zero records. */
typedef struct fpe_opt_out {
    fpe_opt_foothold* footholds; /* [B * n_cycles * 4] */
    fpe_opt_cycle* cycles;       /* [B * n_cycles] */
    uint8_t* gate_fail_cycle;    /* [B] first cycle whose getGaitCycleSearchGridMap failed — the cycle in which the
                                    reference's service handler returns false (cpp:931-934); 255 = none */
    double* rows_after;          /* [B * 2] lfCurrentRow, rhCurrentRow as the call leaves them (cpp:1561-1568: gaitMap_.getIndex
                                    of the committed LF / RH positions; unchanged by cycles that do not commit): what the
                                    NEXT call's fpe_opt_params.lf/rh_current_row0 must be (file-scope globals, cpp:36) */
} fpe_opt_out;

/* One open-loop checkFoothold call (hpp:94-100) with an arbitrary polygon (grid_map::Polygon). */
#define FPE_MAX_POLYGON_VERTICES 8
typedef struct fpe_leg_query {
    double cx, cy;       /* center */
    float search_radius; /* searchRadius */
    int32_t n_vertices;
    double vx[FPE_MAX_POLYGON_VERTICES], vy[FPE_MAX_POLYGON_VERTICES];
} fpe_leg_query;

/* foothold_planner_msgs/Foothold (Foothold.msg:1-3) and foothold_planner_msgs/GlobalFootholds
 * (GlobalFootholds.msg:1-5) as filled by globalFootholdPlan (cpp:591-699, 1378-1396, 1574, 1588):
 * 4 stance entries (gait_cycle_id 0) then 4 per VALID cycle (gait_cycle_id = cycle index). */
typedef struct fpe_msg_foothold {
    double x, y, z;        /* geometry_msgs/Point point */
    uint8_t foot_id;       /* 0 RF, 1 RH, 2 LH, 3 LF */
    uint8_t gait_cycle_id;
    uint8_t pad[6];
} fpe_msg_foothold;
typedef struct fpe_global_footholds {
    uint8_t success;             /* validity of the LAST cycle (cpp:1380, 1574) */
    uint8_t gait_cycles;         /* request.gait_cycles (cpp:592-593) */
    uint8_t gait_cycles_succeed; /* index+1 of the last valid cycle (cpp:1379) */
    uint8_t pad;
    int32_t n_footholds;         /* entries used in `footholds` */
    fpe_msg_foothold footholds[4 + 4 * 255];
} fpe_global_footholds;

/* ---- lifecycle ---------------------------------------------------------------------------- */
/* One engine per process per GPU (device_id = LOCAL_RANK under torch.distributed). */
int fpe_create(int device_id, fpe_handle* out);
int fpe_destroy(fpe_handle h);
/* Build-defined tuning / test knobs of one engine (never read from the environment per call; the
 * environment variables FPE_PLAN_GROUP, FPE_LITERAL_DISCS, FPE_NO_MID_VARIANT, FPE_NO_BITS only seed the
 * defaults once, in fpe_create).  Keys: "plan_group" (0 automatic; 4/8/16/64 lanes per leg, 65 = one
 * wavefront per pose), "literal_discs" (1: force the literal CircleIterator walk), "no_mid_variant"
 * (1: never launch the 3x3-only kernel variants), "no_bits" (1: never launch the bit-window kernels),
 * "service_opt_gate" — what the fpe_plan_service* calls do about the gate of gait cycles >= 1, whose x side follows the
 * opt track's feet, i.e. the BUILD-DEFINED optimiser (see fpe_service_gate below): 2 (DEFAULT) enforce — the opt track's
 * chain runs next to the plan (its own stream) and the call returns FPE_E_SERVICE_FALSE on its verdict too, as the
 * reference's handler does at that gate whatever its optimiser (cpp:920-934); 1 advisory: the chain runs, its verdict is
 * reported by fpe_last_service_gate, the return value stays optimiser-independent; 0: the chain is not run for the gate
 * (latency-critical callers: 48 us instead of 110 us per call; it still runs when an opt product is asked for) and the call
 * returns FPE_E_SERVICE_FALSE only on the optimiser-independent failures.  In modes 0 and 1 a call whose chain stopped at
 * its gate still answers FPE_OK with the nominal / centroid / default products, but the OPT products (message, report, the
 * opt points of the centroid path) come back EMPTY — never the truncated track of an aborted chain — and
 * fpe_last_service_gate names kind FPE_GATE_BUILD_DEFINED and the cycle: a caller that wants the handler's behaviour checks
 * fail_kind, not only the return value.  "service_cycle0_gate_only" (older name): 1 = service_opt_gate 0, 0 = 2.
 * "beam_check_waves": the wavefronts per candidate of the checked beam's check kernel (fpe_plan_beam_checked*): 0 (DEFAULT) by the
 * map's resolution, 1 or 4 forced; the outputs do not depend on it.
 * "scan_merge": the form of the two point passes of fpe_scan_fuse*: 0 (DEFAULT) the engine's choice, 1 plain, 2 merged (see there);
 * the outputs do not depend on it.
 * "scan_clear_form": the form of the ray pass of fpe_scan_clear*: 0 (DEFAULT) the engine's choice, 1 one lane per ray, 2 a group of
 * adjacent lanes per ray; "scan_clear_group": that group's width: 0 (DEFAULT) the engine's choice, 16, 32 or 64 (see there); the
 * outputs depend on neither.
 * "scan_close_form": the form of fpe_scan_close*'s kernel: 0 (DEFAULT) the engine's choice, 1 direct, 2 tiled in LDS (see there); the
 * outputs do not depend on it.
 * "service_overlap" (default 1): a call that runs the plan AND the opt track for at most four poses launches the opt
 * track's chain on a second stream beside the plan kernel, on nominal cycle flags of 1 (the flags only decide which cycles the
 * chain commits, cpp:1323-1332, and are 1 unless a nominal search fails), and runs it again on the real flags in the call where
 * they differ: the same products as 0 (one kernel after the other), the plan kernel's time off the common call's latency.
 * "service_poll" (default 1): in such a call for ONE pose the chain's last instruction writes a completion word into the
 * call's pinned arena (after a system-scope fence behind its product stores) and the host polls that word instead of waiting
 * for the stream's completion signal — the end-of-kernel processing and the wake-up of a stream wait cost several microseconds
 * of a ~100 us call; bounded: after 5 ms without the word the ordinary stream synchronisation takes over.  0: stream waits only.
 * Thread-safe: every plan / search call copies the knobs once, under the engine's lock, so a concurrent call runs
 * entirely with the values before or entirely with the values after a change (one key per call: callers that change
 * several keys while other threads plan get each key's change at its own moment). */
int fpe_set_tuning(fpe_handle h, const char* key, int32_t value);
const char* fpe_last_error(fpe_handle h); /* thread-local text of the last failure on this thread */
const char* fpe_version(void);
/* Layout version of the structs this header passes by pointer (fpe_plan_out, fpe_opt_out, fpe_params, ... have no size
 * field: fields are only ever APPENDED, and every append bumps this number).  A host compiled against this header checks
 * fpe_abi_version() == FPE_ABI_VERSION once after loading the library — a library that reads a longer struct than the host
 * passes would take whatever lies behind it for a device pointer (csrc/ros_adapter/fpe_ros_adapter.hpp and _capi.py do).
 * A NEW struct with new entry points (fpe_stride and the fpe_*_strides* calls) is not an append to an existing struct: it leaves
 * every layout a version-5 host passes as it was, so the number stays 5. */
#define FPE_ABI_VERSION 5
int fpe_abi_version(void);

/* ---- map ingest: replaces GridMapRosConverter::fromMessage in gridmapCallback (cpp:504-536) ---
 * Host pointers, `rows*cols` floats per layer in desc->storage_order.  Uploads both layers to HBM
 * once, canonicalised (row-major, start index 0); the new snapshot becomes current atomically. */
int fpe_upload_map(fpe_handle h, const fpe_map_desc* desc, const float* traversability, const float* elevation);
/* Same with DEVICE pointers (e.g. a map RCCL-broadcast from rank 0); async on `stream`.  Ordering is the
 * engine's job, not the caller's: a plan / search on ANY stream waits (GPU-side) for the upload of the snapshot it
 * uses, and the layer buffers of a snapshot retired while asynchronous launches may still read it are recycled only
 * behind a device synchronisation performed by the NEXT upload — plans never pay for it: the upload also builds the
 * search bit planes for the threshold pairs the previous snapshot was planned with, and a plan that needs planes for
 * a pair never seen before allocates fresh memory rather than wait for a recycled buffer. */
int fpe_upload_map_device(fpe_handle h, const fpe_map_desc* desc, const float* d_traversability,
                          const float* d_elevation, void* stream);
int fpe_map_info(fpe_handle h, fpe_map_desc* out); /* geometry of the current snapshot */

/* ---- incremental map updates: the current snapshot shifted by whole cells, a few rectangles replaced ------------------------
 * BUILD-DEFINED seam for a robot-centric map (elevation_mapping moves its map with grid_map::move: from one message to the next
 * almost every cell keeps its value and only changes its index).  Instead of both full layers, the caller names the shift and hands
 * over the rectangles whose values are new; one streaming pass on the device reads the old canonical layers and writes the new
 * ones together with the bit planes.  Only the patches cross the host link.
 *  - Content.  The base is the snapshot current at entry: rows, cols, resolution, canonical layers T0, E0.  The new snapshot has the
 *    same size and resolution, position u->position, start index (0, 0), row-major.  For every cell (i, j), in this order:
 *      1. if (i + sr, j + sc) lies inside the map, both layers take the base's value there, bit for bit;
 *      2. otherwise both take the quiet NaN 0x7FC00000 (grid_map's cleared cell);
 *      3. patches 0 .. n_patches - 1 are written over that in order: where two patches overlap, the later one wins.
 *    |sr| >= rows or |sc| >= cols is valid: nothing is carried.
 *  - Equivalence.  After the call every entry point behaves byte for byte as if fpe_upload_map had been called with those composed
 *    canonical layers and {rows, cols, resolution, u->position, start (0,0), row-major} — fpe_map_info included.  The planes of
 *    every threshold pair the base snapshot held are rebuilt for the new content in the same pass ("plans never pay for it" keeps
 *    holding); a pair the base never saw is built lazily, as after an upload.  The engine derives nothing about the position from
 *    shift and resolution: it takes the caller's doubles, so the geometry is rounded once, by the caller's grid_map.
 *  - Where shift comes from.  It is the un-wrapped start-index difference of the circular buffer: canonical row i lives in buffer
 *    row (i + s) mod rows, so a buffer whose start index goes from s_old to s_old + d, before wrapping, has shift = d — the index
 *    shift grid_map::move computes (columns alike).  INTEGRATION.md shows the binding.
 *  - Patch sources.  Element (r, c) of a rectangle lies at r * row_stride + c * col_stride, in floats, in one of two forms:
 *    row-major with a pitch (col_stride == 1, row_stride >= n_cols), or column-major with a pitch (row_stride == 1, col_stride >=
 *    n_rows) — a patch may point straight into a non-wrapping region of a column-major message buffer, which is what move's
 *    newRegions are.  Anything else is refused.  Host sources may be freed on return, device sources once `stream` has passed
 *    the call.
 *  - Snapshot semantics: the upload's.  A plan that entered before the update keeps the base; the new snapshot becomes current
 *    atomically; consumers on other streams wait GPU-side for its ready event; the update's own stream waits GPU-side for the base's
 *    upload.  The device form reads the base asynchronously, so the base counts as read by an asynchronous launch (its buffers are
 *    recycled only behind a device synchronisation of a later upload or update); no reference to the base outlives the call: there
 *    is no chain of snapshots.  Updates of one engine serialise among themselves.  An update racing a full upload from another
 *    thread: each is internally consistent, and the last to install wins.  The host form returns with the snapshot and its planes
 *    complete, like fpe_upload_map.
 *  - Refusals (nothing installed, queued or written).  FPE_E_NO_MAP before any upload.  FPE_E_INVALID_ARG for a null handle or
 *    update, n_patches outside 0..FPE_UPDATE_MAX_PATCHES, reserved != 0, a non-finite position, an empty rectangle or one reaching
 *    outside the map, a null layer pointer in a used patch, a stride pair of neither form.  fpe_map_update_validate is that same
 *    routine without an engine: of `base` only rows and cols are read.
 * Out of scope: a change of size or resolution (a full upload).  The producer's filters on the dirty region only are
 * fpe_update_elevation* below. */
#define FPE_UPDATE_MAX_PATCHES 8
typedef struct fpe_map_patch {        /* 48 bytes */
    int32_t row0, col0, n_rows, n_cols;   /* rectangle in canonical indices of the NEW map; non-empty, inside it */
    const float* traversability;          /* element (r, c) of the rectangle at r * row_stride + c * col_stride */
    const float* elevation;               /* same strides */
    int64_t row_stride, col_stride;       /* in floats; one of the two forms above */
} fpe_map_patch;
typedef struct fpe_map_update {       /* 416 bytes */
    int32_t shift[2];      /* (sr, sc): new canonical cell (i, j) carries old canonical cell (i + sr, j + sc) */
    double  position[2];   /* getPosition() of the new map */
    int32_t n_patches;     /* 0..FPE_UPDATE_MAX_PATCHES */
    int32_t reserved;      /* 0 */
    fpe_map_patch patch[FPE_UPDATE_MAX_PATCHES];
} fpe_map_update;
int fpe_update_map(fpe_handle h, const fpe_map_update* u);                       /* patch pointers: HOST; synchronous */
int fpe_update_map_device(fpe_handle h, const fpe_map_update* u, void* stream);  /* `u` on the host, patch pointers: DEVICE; asynchronous */
int fpe_map_update_validate(const fpe_map_desc* base, const fpe_map_update* u);  /* host arithmetic only; no engine */

/* ---- the producer of the map: elevation layer -> traversability layer -----------------
 * The reference starts leggedrobotics/traversability_estimation (launch/mapping.launch:12-13,
 * launch/all.launch:21-22, README.md:29) and subscribes to its output (cpp:188); package and filter
 * configuration are not part of the reference, no version is pinned.  These entry points restate that package's
 * published default chain (grid_map_filters NormalVectorsFilter, area method; SlopeFilter, StepFilter,
 * RoughnessFilter; traversability = (1/3)(slope + step + roughness) on float layers) as disc stencils on the
 * device, so that `elevation message -> traversability -> fpe_upload_map_device -> fpe_plan_device` never leaves
 * HBM.  PARITY UNPINNED: the arithmetic contract is the build's own oracle (oracle/fpo_filters.cpp). */
typedef struct fpe_filter_params {
    double normal_radius;        /* NormalVectorsFilter radius [m]                      (0.05) */
    double slope_critical;       /* SlopeFilter critical_value [rad]                    (1.0)  */
    double step_critical;        /* StepFilter critical_value [m]                       (0.12) */
    double step_first_radius;    /* StepFilter first_window_radius [m]                  (0.08) */
    double step_second_radius;   /* StepFilter second_window_radius [m]                 (0.08) */
    int32_t step_critical_cells; /* StepFilter critical_cell_number                     (4)    */
    int32_t reserved;
    double roughness_critical;   /* RoughnessFilter critical_value [m]                  (0.05) */
    double roughness_radius;     /* RoughnessFilter estimation_radius [m]               (0.05) */
} fpe_filter_params;
int fpe_filter_params_defaults(fpe_filter_params* out);
#define FPE_FILTER_LAYERS 8 /* surface_normal_x, _y, _z, traversability_slope, step_height, traversability_step,
                               traversability_roughness, traversability — each rows*cols floats */
/* Host buffers: `elevation` in desc's layout (storage order, start index); `traversability` (required) and `layers`
 * (optional, FPE_FILTER_LAYERS * rows * cols floats) come back CANONICAL (row-major, start index 0).  Synchronous. */
int fpe_traversability(fpe_handle h, const fpe_map_desc* desc, const fpe_filter_params* fp, const float* elevation,
                       float* traversability, float* layers);
/* Device buffers, asynchronous on `stream`; d_layers optional (scratch from the engine's pool when null).
 * Several producers may call on different streams concurrently (the reference's callbacks run under AsyncSpinner(0),
 * foothold_planner_node.cpp:12): no call synchronises the device or blocks the host — the engine keeps up to four
 * internal step-height buffers, each guarded by an event recorded behind the chain that used it last; a fifth concurrent
 * stream waits GPU-side for the least recently used one.  `stream` must outlive the chains queued on it. */
int fpe_traversability_device(fpe_handle h, const fpe_map_desc* desc, const fpe_filter_params* fp, const float* d_elevation,
                              float* d_traversability, float* d_layers, void* stream);

/* ---- elevation-driven map updates: the producer's filters on the dirty region only ---------------------------------------------
 * BUILD-DEFINED.  fpe_update_map's shift and patches, with patches that carry ELEVATION only: one call composes the new elevation
 * layer (fpe_update_map's steps 1-3 applied to the elevation), runs the filter chain above over the tiles whose input changed,
 * lets the shift carry every other cell's traversability, rebuilds the bit planes and installs the snapshot.
 *  - `u`: shift, position, patch count, rectangles and stride forms mean what they mean for fpe_update_map.  patch[k].elevation is
 *    required; patch[k].traversability must be NULL (FPE_E_INVALID_ARG).  Every other refusal of fpe_update_map applies unchanged;
 *    a parameter set fpe_traversability* would refuse returns what it returns there (FPE_E_UNSUPPORTED for radii beyond the stencil
 *    tables).  A refused call installs, queues and writes nothing.  fp == NULL: the defaults.  info may be NULL.
 *  - Reach.  R = max(hN, hR, h1 + h2), h* = int(radius / resolution) + 1 of the normals, roughness, first and second step radius:
 *    10 cells with the defaults at 2 cm.  fpe_filter_reach_cells returns it (FPE_E_INVALID_ARG < 0 for bad arguments).
 *  - Dirty set D.  In the new map's canonical indices, with shift (sr, sc):
 *      C holds the cells of every patch rectangle, and every cell without a source, meaning that (i + sr, j + sc) lies outside
 *        the map.
 *      B holds carried cells whose window is clipped differently by the map edge before and after the move.  If sr != 0, these are
 *        the rows i with i < R, or i >= rows - R, or i + sr < R, or i + sr >= rows - R.  If sc != 0, the columns follow the same
 *        rule.
 *      D = {cells within Chebyshev distance R of a cell of C} united with B, clipped to the map.
 *  - Content.  Let E* be the composed elevation and F what fpe_traversability_device writes for E* with the new map's geometry
 *    {rows, cols, resolution, u->position, start (0,0), row-major} and d_layers == NULL — the traversability-only chain (it and the
 *    all-layers chain are not bit-identical to each other; F is the former).  After the call the snapshot's elevation is E*, and its
 *    traversability T* satisfies, bit for bit: every cell of D holds F; every other cell holds either F or the base snapshot's value
 *    at (i + sr, j + sc), whatever produced that value; the set of cells the chain stored has recomputed_cells elements, contains D,
 *    and is a function of the inputs alone (the chain stores whole tiles of its global tile grid, without a store mask).
 *    NOT PROMISED: a carried value is the filter's answer at the OLD position and tile alignment — it is not re-derived at the new
 *    position, and it is not byte-equal to a fresh run in the last place (the row-moment prefix differences depend on the tile
 *    alignment, the lattice shapes on the map's distance from the origin).  A changed fpe_filter_params between updates is the
 *    caller's business: carried cells keep what they hold.
 *  - Routes.  route 0: region launches of the chain's two kernels over the dirty tiles.  route 1, NOT a partial update: where the
 *    chain for these parameters and this geometry is not the two-launch traversability-only one (roughness radius != normal radius,
 *    the published windows at 0.5 cm, a map too far from the origin for the lattice forms), or |shift| >= the map's size, the full
 *    chain runs over the whole composed map; every cell then holds F and recomputed_cells = rows * cols.
 *  - Everything else behaves byte for byte as if fpe_upload_map had been called with (T*, E*) and the new geometry: fpe_map_info,
 *    the planes of every threshold pair the base held (rebuilt from T* behind the chain), lazily built planes for new pairs, and
 *    fpe_update_map's snapshot semantics — a plan that entered before keeps the base, installation is atomic, updates (of either
 *    kind) serialise among themselves, the device form never synchronises the host, the base counts as read by an asynchronous launch.
 *  - fpe_elevation_update_plan: the validation and the dirty set without an engine; of `base` rows, cols, resolution are read (the
 *    new position is u->position).  dirty: rows * cols bytes, 1 for the cells of D. */
int fpe_filter_reach_cells(const fpe_filter_params* fp, double resolution);   /* host arithmetic; no engine */
typedef struct fpe_elevation_update_info {
    int32_t reach_cells;       /* R */
    int32_t route;             /* 0 = region launches, 1 = the full chain over the whole map (fallback) */
    int64_t dirty_cells;       /* |D| */
    int64_t recomputed_cells;  /* cells whose traversability the chain stores: >= dirty_cells */
} fpe_elevation_update_info;
int fpe_elevation_update_plan(const fpe_map_desc* base, const fpe_filter_params* fp, const fpe_map_update* u,
                              fpe_elevation_update_info* info /* may be NULL */, uint8_t* dirty /* [rows*cols] 0/1, may be NULL */);
int fpe_update_elevation(fpe_handle h, const fpe_filter_params* fp, const fpe_map_update* u, fpe_elevation_update_info* info);  /* patch pointers: HOST; synchronous */
int fpe_update_elevation_device(fpe_handle h, const fpe_filter_params* fp, const fpe_map_update* u,
                                fpe_elevation_update_info* info, void* stream);  /* `u` on the host, patch pointers: DEVICE; asynchronous */

/* The canonical layers of the snapshot current at entry, bit for bit: row-major, start index (0, 0), rows * cols floats each.
 * Either pointer may be NULL, not both.  Snapshot semantics of fpe_plan; the device form waits GPU-side for the snapshot's upload
 * and never synchronises the host. */
int fpe_read_map_layers(fpe_handle h, float* traversability, float* elevation);                       /* host; synchronous */
int fpe_read_map_layers_device(fpe_handle h, float* d_traversability, float* d_elevation, void* stream);

/* Name and shape of the kernel a chained plan with these parameters launches on the current map (evidence for
 * benchmarks and profiles; e.g. "plan_bits_kernel<2, true> (8 lanes per leg, 13 x 13 bit window, 3x3-only fast path)"). */
int fpe_describe_plan(fpe_handle h, const fpe_params* params, char* buf, int32_t n);

/* Build-defined: upper bound of fpe_pose.leg_search_radius the device-resident entry points size
 * their LDS tile for (the host-buffer entry points scan the poses themselves).  Default 0 =
 * fpe_params.searchRadius only; legs asking for more come back invalid with source = 3. */
int fpe_set_max_leg_search_radius(fpe_handle h, float radius);

/* ---- chained plan: replaces the body of the per-cycle loop of globalFootholdPlan (cpp:762-1579)
 * — getDefaultFootholds, getFootholdSearchGridMap, 4x checkFootholdUseCentroidMethod (cpp:818-821),
 * 4x std::thread(checkFoothold) + join (cpp:863-909), the commit rule (cpp:1323-1576) and the
 * lateral drift (cpp:1578) — for B independent initial poses.  The "opt" track (cpp:913-1319) does not feed
 * these products; it is a launch of its own (fpe_plan_opt*). */
int fpe_plan(fpe_handle h, const fpe_params* params, const fpe_pose* poses, int32_t B, int32_t n_cycles,
             const fpe_plan_out* out);
/* Host arrays the GPU can write by DMA (pinned).  fpe_plan / fpe_plan_opt copy a product whose destination lies in such
 * memory — allocated here, by hipHostMalloc or registered with hipHostRegister — from the device straight into it;
 * other destinations are served through the engine's own pinned arena and a copy (overlapped, chunk by chunk).  A ROS
 * adapter that keeps its result arrays across service calls allocates them once with fpe_host_alloc.  Products whose
 * pinned destinations lie directly behind one another in the order of fpe_plan_out's fields (nominal, centroid, default_next,
 * cycle_ok, stance, selected, pose_status; no gap, sizes that are multiples of 256 bytes) leave in ONE transfer: carve them
 * out of one block in that order (a transfer has a fixed cost of some ten microseconds). */
int fpe_host_alloc(fpe_handle h, size_t bytes, void** out);
int fpe_host_free(fpe_handle h, void* p);

/* Device-resident variant: d_poses and every non-NULL pointer of d_out are DEVICE pointers; the
 * launch is asynchronous on `stream` (a hipStream_t; NULL = default stream). */
int fpe_plan_device(fpe_handle h, const fpe_params* params, const fpe_pose* d_poses, int32_t B,
                    int32_t n_cycles, const fpe_plan_out* d_out, void* stream);

/* ---- the opt track of the same batch: replaces cpp:913-1319 + cpp:1485-1568 of the cycle loop ----------------
 * cycle_ok = fpe_plan_out.cycle_ok of the SAME poses / parameters / map (the opt track commits with the nominal
 * track's validity, cpp:1323-1332).  Host variant: cycle_ok may be NULL — the engine then runs the chained plan
 * itself first.  Device variant: asynchronous on `stream`, ordered after the plan launch that wrote d_cycle_ok. */
int fpe_plan_opt(fpe_handle h, const fpe_params* params, const fpe_opt_params* opt, const fpe_pose* poses, int32_t B,
                 int32_t n_cycles, const uint8_t* cycle_ok, const fpe_opt_out* out);
int fpe_plan_opt_device(fpe_handle h, const fpe_params* params, const fpe_opt_params* opt, const fpe_pose* d_poses,
                        int32_t B, int32_t n_cycles, const uint8_t* d_cycle_ok, const fpe_opt_out* d_out, void* stream);

/* ---- open-loop per-leg search: replaces checkFoothold (cpp:2001-2036) one call per query ------ */
int fpe_search_legs(fpe_handle h, const fpe_params* params, const fpe_leg_query* queries, int32_t n,
                    fpe_foothold* out);
int fpe_search_legs_device(fpe_handle h, const fpe_params* params, const fpe_leg_query* d_queries, int32_t n,
                           fpe_foothold* d_out, void* stream);

/* ---- service-shaped call: one pose, response content of plan_global_footholds (cpp:539-1602) --
 * The reference's handler returns false when getGaitCycleSearchGridMap's getSubmap fails (cpp:920-934, 2345-2349) — in
 * ANY gait cycle.  That submap is centred at (x of the opt track's next feet centre, initialPose_[1] + ajustedPose_[1]):
 *   * in gait cycle 0 the feet are the stance: exact, decided by the plan kernels (FPE_POSE_OPT_SUBMAP_FAILED);
 *   * its y side depends on the cycle number only (the lateral drift, cpp:1578): exact in EVERY cycle, decided on the
 *     host with the same grid arithmetic — a request whose y side fails in some cycle g < gait_cycles is refused by the
 *     reference in cycle g at the latest, whatever its optimiser does;
 *   * its x side in cycles >= 1 follows the opt track's feet, i.e. NLopt's COBYLA iterates (cpp:1116-1211), which this
 *     build cannot reproduce (fpe_opt_params): BUILD-DEFINED, advisory by default.
 * These calls return FPE_E_SERVICE_FALSE (response zeroed) on the first two kinds always, on the third under
 * fpe_set_tuning("service_opt_gate", 2) — the default.  fpe_last_service_gate tells the kinds apart. */
typedef struct fpe_service_gate {
    uint8_t fail_cycle;  /* gait cycle in which the handler's gate fails; 255 = it never does */
    uint8_t fail_kind;   /* FPE_GATE_* */
    uint8_t chain_ran;   /* the opt track's chain was run for this call (its verdict is known) */
    uint8_t returned_false; /* the call returned FPE_E_SERVICE_FALSE */
    uint8_t pad[4];
    double lf_current_row, rh_current_row; /* chain_ran: lfCurrentRow / rhCurrentRow as the call leaves them
                                              (fpe_opt_out.rows_after): the adapter carries them into the next call */
} fpe_service_gate;
#define FPE_GATE_NONE 0          /* no failing cycle (x side of cycles >= 1 unknown when chain_ran = 0) */
#define FPE_GATE_CYCLE0 1        /* exact: first gait cycle, stance feet */
#define FPE_GATE_LATERAL 2       /* exact: y side of cycle fail_cycle (lateral drift), optimiser-independent */
#define FPE_GATE_BUILD_DEFINED 3 /* x side of a cycle >= 1: follows the build-defined optimiser's feet */
/* Gate verdict of the last fpe_plan_service* call made on THIS thread with engine h. */
int fpe_last_service_gate(fpe_handle h, fpe_service_gate* out);
int fpe_plan_service(fpe_handle h, const fpe_params* params, const double initial_position[3],
                     uint8_t gait_cycles, fpe_global_footholds* response);

/* Same call, plus the other two result products the node publishes/logs; either
 * extra pointer may be NULL.
 *   centroid: content of global_footholds_centroid for THIS call (cpp:709-727 stance entries,
 *             cpp:1444-1462 per valid cycle; the reference never clears that message between
 *             calls, cpp:715 — appending across calls is left to the adapter).  Its bookkeeping is NOT
 *             the nominal one: success = 1 iff any cycle committed (set false once at cpp:711, true at
 *             cpp:1446, never cleared by a later failed cycle — cpp:1574 touches the nominal message
 *             only), gait_cycles_succeed = last committed cycle + 1, gait_cycles is never written (0);
 *   default_footholds: rows of globalFootholdsResult_.defaultFootholds (cpp:666-671, 1344-1348):
 *             (1 + gait_cycles_succeed') x 12 doubles = RF,RH,LH,LF x (x,y,z), stance row first, one row
 *             per VALID cycle; *n_default_rows receives the number of rows (capacity 1 + gait_cycles). */
int fpe_plan_service_ex(fpe_handle h, const fpe_params* params, const double initial_position[3],
                        uint8_t gait_cycles, fpe_global_footholds* response, fpe_global_footholds* centroid,
                        double* default_footholds, int32_t* n_default_rows);

/* Evaluation products of one track of a service call:
 *   feet_center_path: poses of nominal_feet_center_path / centroid_feet_center_path (cpp:231-232,
 *             1410, 1477): getPolygonCenter of the track's CURRENT feet, one per planned cycle whether
 *             or not it commits (getFootholdSearchGridMap, cpp:2191-2196);
 *   feet_distance / cog_speed: footholdsKPI_ (hpp:732-745), two entries per COMMITTED cycle
 *             (getHipDistance cpp:2571-2584, getCogSpeed cpp:2587-2623 with gaitCycle_ = 1.0, cpp:332). */
typedef struct fpe_track_report {
    int32_t n_path; /* nominal: gait_cycles.  centroid: 2 x gait_cycles — the opt track's getFootholdSearchGridMap call is
                       handed centroidFeetCenterPath too (cpp:946), so every cycle appends the centroid track's centre
                       and then the opt track's */
    int32_t n_kpi;  /* = 2 x committed cycles */
    double feet_center_path[2 * 255][3];
    double feet_distance[2 * 255];
    double cog_speed[2 * 255];
} fpe_track_report;
/* fpe_plan_service_ex plus the per-track reports; every pointer after `response` may be NULL. */
int fpe_plan_service_report(fpe_handle h, const fpe_params* params, const double initial_position[3],
                            uint8_t gait_cycles, fpe_global_footholds* response, fpe_global_footholds* centroid,
                            double* default_footholds, int32_t* n_default_rows, fpe_track_report* nominal_report,
                            fpe_track_report* centroid_report);

/* fpe_plan_service_report plus the opt track's products; every pointer after `response` may be
 * NULL, `opt` NULL = fpe_opt_params_yaml.
 *   opt_msg:    content of global_footholds_opt for THIS call (cpp:737-755 stance entries, cpp:1510-1532 per committed
 *               cycle; bookkeeping as the centroid message: success = any cycle committed, gait_cycles never written);
 *   opt_report: footholdsKPI_.feetDistance_opt / cogSpeed_opt (cpp:1488-1499); feet_center_path holds the opt
 *               track's feet centres (the entries it interleaves into the centroid path);
 *   opt_cycles: [gait_cycles] the per-cycle problems and solutions. */
int fpe_plan_service_opt(fpe_handle h, const fpe_params* params, const fpe_opt_params* opt, const double initial_position[3],
                         uint8_t gait_cycles, fpe_global_footholds* response, fpe_global_footholds* centroid,
                         double* default_footholds, int32_t* n_default_rows, fpe_track_report* nominal_report,
                         fpe_track_report* centroid_report, fpe_global_footholds* opt_msg, fpe_track_report* opt_report,
                         fpe_opt_cycle* opt_cycles);

/* ---- several GPUs in ONE process (fpe_multi.cpp) ----------------------------------------------
 * north_star: "a batch of candidate body trajectories is the parallel axis and shards across the 8 GPUs of one
 * node".  A C++ host that owns every GPU of the node (the ROS node) creates one group: an engine per device, the
 * map replicated by fpe_multi_upload_map, and fpe_multi_plan splitting the pose batch into contiguous blocks (the
 * first B % n devices take one pose more), one resident host thread per device, results written into the caller's
 * arrays at their global positions.  (A group may list one device several times — independent engines — for the
 * host-buffer form; the RCCL form needs distinct devices.)  Same semantics, argument meaning and status codes as the single-device calls they
 * fan out to (fpe_upload_map, fpe_plan: the seam at cpp:863-909 for every pose of the batch).  The
 * one-process-per-GPU deployment (torch.distributed + RCCL all-gather of fpe_plan_out.selected) uses the
 * single-device entry points instead (bench.py, quadrupedal_foothold_planner_amd/dist.py). */
typedef struct fpe_multi* fpe_multi_handle;
int fpe_multi_create(const int32_t* device_ids, int32_t n_devices, fpe_multi_handle* out);
int fpe_multi_destroy(fpe_multi_handle h);
int fpe_multi_device_count(fpe_multi_handle h);
fpe_handle fpe_multi_engine(fpe_multi_handle h, int32_t k); /* engine of device k (for the single-device calls) */
const char* fpe_multi_last_error(fpe_multi_handle h);
int fpe_multi_upload_map(fpe_multi_handle h, const fpe_map_desc* desc, const float* traversability,
                         const float* elevation);
/* fpe_update_map (the host form) on every engine of the group; every engine must hold a map of the same size */
int fpe_multi_update_map(fpe_multi_handle h, const fpe_map_update* u);
int fpe_multi_set_tuning(fpe_multi_handle h, const char* key, int32_t value);
int fpe_multi_plan(fpe_multi_handle h, const fpe_params* params, const fpe_pose* poses, int32_t B, int32_t n_cycles,
                   const fpe_plan_out* out);
/* Block of device k of a batch of B poses split over n_devices: poses [*first, *first + *count). */
int fpe_multi_shard_range(int32_t B, int32_t k, int32_t n_devices, int32_t* first, int32_t* count);

/* Device-resident form with the xGMI all-gather north_star names, for the C++ host that owns every GPU of the node
 * (replaces the 4 std::thread + join of cpp:863-909 for every pose of the batch, on all devices at once).  io[k]
 * describes device k: its block's poses and products in ITS memory (block = fpe_multi_shard_range(B, k, n)), its
 * stream (NULL: the group's own stream of that device, fpe_multi_stream), and — when record_kind is not
 * FPE_EXCHANGE_NONE — d_gathered: room for the records of the WHOLE batch in pose order, [B * n_cycles * 4] records of
 * the chosen kind.  The call queues, per device, the plan of its block and then ONE fused RCCL collective
 * (ncclGroupStart / ncclAllGather per device / ncclGroupEnd) on the same streams; when B % n != 0 the blocks travel PADDED
 * to ceil(B / n) poses through a staging buffer of the group (in-place all-gather) and n device-local copies put them at
 * their places: d_gathered on every device holds every block's records once its stream has passed the call.  Nothing
 * synchronises the host.  RCCL is loaded at the first gathering call (librccl.so.1); FPE_E_UNSUPPORTED without it. */
#define FPE_EXCHANGE_NONE 0
#define FPE_EXCHANGE_SELECTED 1 /* fpe_selected_foothold, 16 bytes: d_out.selected is the block's contribution */
#define FPE_EXCHANGE_PACKED 2   /* fpe_selected_packed, 8 bytes: d_out.selected_packed */
typedef struct fpe_multi_device_io {
    const fpe_pose* d_poses; /* device k's block of poses */
    fpe_plan_out d_out;      /* device k's products of its block (device pointers; any may be NULL) */
    void* d_gathered;        /* device k: records of the whole batch, or NULL with FPE_EXCHANGE_NONE */
    void* stream;            /* hipStream_t of device k, or NULL */
} fpe_multi_device_io;
int fpe_multi_plan_device(fpe_multi_handle h, const fpe_params* params, const fpe_multi_device_io* io, int32_t B, int32_t n_cycles,
                          int32_t record_kind);
void* fpe_multi_stream(fpe_multi_handle h, int32_t k); /* the group's own stream of device k (a hipStream_t) */
int fpe_multi_synchronize(fpe_multi_handle h);          /* waits for the group's own streams */

/* ---- dense foothold map: the reference's foot-disc functions at EVERY cell centre of a region -----------------
 * For cell (i, j) of the current snapshot (canonical indices: row-major, start index (0,0), rows span x) with centre
 * p = getPosition(i, j) and disc CircleIterator(map, p, footRadius) — clipped at the map edge, f64 membership test:
 *   FPE_FMAP_DEFAULT_OK   checkDefaultFoothold(p) (cpp:2039-2082, defaultFootholdThreshold): the disc is non-empty and no
 *                         FINITE cell of it is below the threshold (non-finite cells pass);
 *   FPE_FMAP_CANDIDATE_OK checkCirclePolygonFoothold(p) (cpp:2117-2163, candidateFootholdThreshold) with a polygon that
 *                         holds every cell: the spiral candidate test of fpe_search_legs / fpe_plan;
 *   FPE_FMAP_UNKNOWN      build-defined: some in-map cell of the disc has non-finite traversability;
 *   height                getFootholdMeanHeight(p, footRadius, h) (cpp:2520-2554), bit for bit.
 * Discs use the host-proved offset table where it holds and the literal walk elsewhere, as the plan kernels do
 * (fpe_set_tuning "literal_discs" 1 forces the walk).  FPE_E_UNSUPPORTED when the literal walk is needed and
 * ceil(footRadius / resolution) > 32.  Snapshot semantics of fpe_plan; the threshold pair's bit planes are shared with
 * the plan calls.  The host form is synchronous (pinned destinations are written by DMA); the device form is
 * asynchronous on `stream` and waits GPU-side for the snapshot's upload. */
#define FPE_FMAP_DEFAULT_OK 1u
#define FPE_FMAP_CANDIDATE_OK 2u
#define FPE_FMAP_UNKNOWN 4u
typedef struct fpe_foothold_map_out {
    uint8_t* flags; /* [n_rows * n_cols] FPE_FMAP_* bits, or NULL */
    float* height;  /* [n_rows * n_cols] foot-disc mean height, or NULL */
} fpe_foothold_map_out;
/* roi = {row0, col0, n_rows, n_cols} in canonical indices, inside the map; NULL = the whole map.
 * Output element (r, c) = cell (row0 + r, col0 + c), row-major. */
int fpe_foothold_map(fpe_handle h, const fpe_params* params, const int32_t roi[4], const fpe_foothold_map_out* out);
int fpe_foothold_map_device(fpe_handle h, const fpe_params* params, const int32_t roi[4],
                            const fpe_foothold_map_out* d_out, void* stream);

/* ---- dense snap map: checkFoothold's landing cell for EVERY cell of a region -----------------------------------
 * Output element (r, c) is exactly what fpe_search_legs returns for the query of cell (i, j) = (row0 + r, col0 + c) of the
 * current snapshot (canonical indices, as fpe_foothold_map): centre = getPosition(i, j); search_radius (<= 0 means
 * fpe_params.searchRadius); polygon = getSearchPolygon(centre, search_radius) (cpp:2496-2517: vertices LU, RU, RD, LD with
 * r = double(float R) and 0.5 * r) for polygon_kind 0, or the plan kernels' hexagon of fpe_pose.leg_polygon_kind 1.  With
 * that result f:
 *   source  f.source: 0 default-disc hit, 1 spiral candidate, 2 none;
 *   offset  (f.row - i, f.col - j) when source is 1, else (0, 0) (a default hit lands on getIndex(centre) = (i, j); a spiral
 *           hit at ring 0, default failed and candidate passed, is source 1 with offset (0, 0));
 *   z       f.z: getFootholdMeanHeight at the CELL centre (cpp:2029), 0 when source is 2.
 * A radius that fpe_search_legs would report as source 3 (over the tile bound) fails with FPE_E_UNSUPPORTED and writes
 * nothing; a polygon_kind other than 0 or 1 fails with FPE_E_INVALID_ARG.  Any NULL product is skipped (at least one must be
 * given).  roi, snapshot semantics, pinned destinations, the literal_discs tuning and the shared bit planes behave as in
 * fpe_foothold_map; z needs what fpe_foothold_map's height needs.  Where the host proves the rectangle and the spiral's ring
 * filter translation-invariant for this map and radius, the search is a bitwise first-hit dilation of the bit planes; the
 * hexagon and everything else run the per-cell search of fpe_search_legs (same results, per-query speed). */
typedef struct fpe_foothold_snap_out {
    int8_t* offset;  /* [n_rows * n_cols * 2] (di, dj): landing cell = (i + di, j + dj); (0, 0) unless source == 1 */
    uint8_t* source; /* [n_rows * n_cols] fpe_foothold.source: 0 default-disc hit, 1 spiral candidate, 2 none */
    float* z;        /* [n_rows * n_cols] fpe_foothold.z: getFootholdMeanHeight at the cell centre, 0 when source 2 */
} fpe_foothold_snap_out;
int fpe_foothold_snap(fpe_handle h, const fpe_params* params, const int32_t roi[4], float search_radius, int32_t polygon_kind,
                      const fpe_foothold_snap_out* out);
int fpe_foothold_snap_device(fpe_handle h, const fpe_params* params, const int32_t roi[4], float search_radius,
                             int32_t polygon_kind, const fpe_foothold_snap_out* d_out, void* stream);

/* ---- open-loop centroid method: checkFootholdUseCentroidMethod (cpp:1605-1997) one call per query ------------------
 * Each query returns exactly the record the plan kernels write to fpe_plan_out.centroid for a leg centred on (cx, cy) with
 * that search radius: the rectangle {2R, R} around the centre (cpp:1616-1617), the scan of its rows, then the case and the
 * mean foot height of the result.  A centre outside the map or not finite gives code 6 (getSubmap fails).  The host form
 * refuses a non-finite search_radius with FPE_E_INVALID_ARG; the device form gives such a query code 6.  The radius has no
 * upper bound here (the row scan loops).  The device form is asynchronous on `stream` and sees the snapshot current at the
 * call. */
typedef struct fpe_centroid_query {
    double cx, cy;       /* the foothold the method starts from (defaultFoothold, cpp:1605) */
    float search_radius; /* searchRadius_ of the rectangle {2R, R} (cpp:1616-1617); <= 0: fpe_params.searchRadius */
    int32_t pad;
} fpe_centroid_query;    /* 24 bytes */
int fpe_centroid_legs(fpe_handle h, const fpe_params* params, const fpe_centroid_query* queries, int32_t n,
                      fpe_centroid_foothold* out);
int fpe_centroid_legs_device(fpe_handle h, const fpe_params* params, const fpe_centroid_query* d_queries, int32_t n,
                             fpe_centroid_foothold* d_out, void* stream);

/* ---- dense centroid map: the centroid method at EVERY cell centre of a region ------------------------------------------
 * Output element (r, c) is exactly the record the open-loop centroid query returns for the centre getPosition(i, j) of cell
 * (i, j) = (row0 + r, col0 + c) of the current snapshot (canonical indices, as fpe_foothold_map) and search_radius (<= 0
 * means fpe_params.searchRadius), written as:
 *   code    the record's code (0..6);
 *   offset  (row - i, col - j) of the record: the landing cell.  (0, 0) for codes 0, 5 and 6.  The record's exact x / y are
 *           the SUBMAP's getPosition of the result (cpp:1816) and can differ from getPosition(row, col) in the last bits:
 *           callers who need them exactly use the open-loop query;
 *   z       the record's z: the mean foot height at the centre (code 0) or at the result's position (codes 1-4), 0 for 5, 6.
 * A radius whose rectangle reaches more than 100 rows or columns from its cell (ceil(R / res) + 2 > 100) fails with
 * FPE_E_UNSUPPORTED and writes nothing.  Any NULL product is skipped (at least one must be given).  roi, snapshot semantics
 * and pinned destinations behave as in fpe_foothold_map: the host form is synchronous, the device form asynchronous on
 * `stream`.  literal_discs changes nothing: z always comes from the per-query disc functions. */
typedef struct fpe_centroid_map_out {
    uint8_t* code;  /* [n_rows * n_cols] fpe_centroid_foothold.code (0..6) */
    int8_t* offset; /* [n_rows * n_cols * 2] (row - i, col - j) of the result; (0, 0) for codes 0, 5, 6 */
    float* z;       /* [n_rows * n_cols] fpe_centroid_foothold.z; 0 for codes 5, 6 */
} fpe_centroid_map_out;
int fpe_centroid_map(fpe_handle h, const fpe_params* params, const int32_t roi[4], float search_radius,
                     const fpe_centroid_map_out* out);
int fpe_centroid_map_device(fpe_handle h, const fpe_params* params, const int32_t roi[4], float search_radius,
                            const fpe_centroid_map_out* d_out, void* stream);

/* ---- rank a pose batch on the device: per-pose summaries, the best K poses and their products, compacted ----------------
 * BUILD-DEFINED (the reference plans one pose per service call and ranks nothing).  One call plans the batch as fpe_plan does,
 * reduces every pose's plan to a 64-byte summary, scores the poses, and returns the K best pose indices with only those
 * poses' products.  What a summary holds is the reference's own bookkeeping and KPIs, per pose:
 *   success, gait_cycles_succeed   the GlobalFootholds bookkeeping of the nominal message (cpp:1379-1380, 1574), exactly as
 *                         fpe_plan_service derives it from cycle_ok;
 *   cog_speed_*, feet_distance_*   footholdsKPI_ of the nominal track (getHipDistance cpp:2571-2584, getCogSpeed cpp:2587-2623):
 *                         the entries of fpe_track_report of the nominal track — the current feet start at stance - double(stepLength / 2),
 *                         two entries of each per committed cycle, RF_FIRST honoured.  min / max by `v < min` / `v > max` from the
 *                         first entry on; the sum sequential in report order.  Trot only: walk-gait poses have all five 0;
 *   deviation_sq_sum      over every cycle g with cycle_ok, ascending, legs RF, RH, LH, LF: acc = acc + (dx*dx + dy*dy) with
 *                         dx = nominal.x - default_next.x, dy alike (f64, no contraction).
 * score = w_fail*(n_cycles - committed) + w_spiral*n_source[1] + w_none*(n_source[2] + n_source[3]) + w_deviation*deviation_sq_sum
 *         + w_speed_spread*(cog_speed_max - cog_speed_min): each product first, the five terms added left to right in f64, -0.0
 * stored as +0.0.  Order: (class, score, pose index) ascending — class 2 = non-finite score (ordered by index alone), class 1 =
 * gait_cycles_succeed < min_cycles, class 0 = the rest; equal scores (IEEE ==) fall to the index.  The result is a function
 * of the inputs alone: nothing depends on workgroup scheduling. */
typedef struct fpe_pose_summary {          /* 64 bytes */
    uint8_t  success;              /* nominal message: validity of the LAST cycle (cpp:1380, 1574) */
    uint8_t  gait_cycles_succeed;  /* index + 1 of the last valid cycle (cpp:1379); 0 = none */
    uint8_t  committed;            /* number of valid cycles */
    uint8_t  first_failed;         /* first cycle with cycle_ok 0; 255 = none */
    uint8_t  pose_status;          /* FPE_POSE_* bits */
    uint8_t  pad[3];
    uint16_t n_source[4];          /* legs of ALL planned cycles by fpe_foothold.source 0..3; sums to 4 * n_cycles */
    double   cog_speed_sum;        /* sum of the nominal track's cog_speed entries, report order, starting from +0.0 */
    double   cog_speed_min, cog_speed_max;         /* over the same entries; 0 when there are none */
    double   feet_distance_min, feet_distance_max; /* over the nominal feet_distance entries; 0 when none */
    double   deviation_sq_sum;     /* see above */
} fpe_pose_summary;

typedef struct fpe_rank_params {
    double  w_fail, w_spiral, w_none, w_deviation, w_speed_spread;  /* all finite, else FPE_E_INVALID_ARG */
    int32_t min_cycles;   /* poses with gait_cycles_succeed < min_cycles are class 1; 0..255 */
    int32_t reserved;
} fpe_rank_params;
/* build-defined defaults: w_fail 100, w_spiral 1, w_none 0, w_deviation 10, w_speed_spread 0, min_cycles 0 */
int fpe_rank_params_defaults(fpe_rank_params* out);

typedef struct fpe_rank_out {
    fpe_pose_summary* summary;   /* [B] or NULL */
    double*  score;              /* [B] or NULL */
    int32_t* best;               /* [K] pose indices, best first — required */
    int32_t* n_class0;           /* [1] number of class-0 poses in the whole batch, or NULL */
    fpe_plan_out best_products;  /* products of pose best[k] in slot k: shapes of fpe_plan_out with B replaced by K;
                                    any pointer may be NULL.  gait_cycle_id / foot_id inside the records stay as planned */
} fpe_rank_out;

/* Replaces, for a node that samples B candidate start poses, B plan_global_footholds calls (cpp:539-1602) and the comparison of
 * their responses on the host: fpe_plan's seam (cpp:762-1579) for the batch, then the pick.  Host arrays; synchronous; only the
 * K-sized and B-sized outputs cross the link (pinned destinations, fpe_host_alloc, are written without a staging copy where the
 * output is large).  rank NULL = fpe_rank_params_defaults.  1 <= K <= min(B, 1024) and 1 <= n_cycles <= 255, else
 * FPE_E_INVALID_ARG; a refused call writes nothing.  The map-size bound of selected_packed (FPE_PACKED_MAX_CELLS) applies only
 * when that product is requested. */
int fpe_plan_rank(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_pose* poses,
                  int32_t B, int32_t n_cycles, int32_t K, const fpe_rank_out* out);
/* Device-resident form of the same seam: d_poses and every non-NULL pointer of d_full / d_out are DEVICE pointers; asynchronous
 * on `stream`, snapshot semantics of fpe_plan_device.  d_full (may be NULL) receives the un-compacted products of all B poses
 * exactly as fpe_plan_device writes them, and the ranking reads them there; products the ranking needs that the caller did
 * not ask for live in stream-ordered scratch. */
int fpe_plan_rank_device(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_pose* d_poses,
                         int32_t B, int32_t n_cycles, int32_t K, const fpe_plan_out* d_full /* may be NULL */,
                         const fpe_rank_out* d_out, void* stream);

/* ---- per-pose stride: step length and lateral drift as a parallel array ---------------------------------------------------------
 * BUILD-DEFINED (the reference has one stepLength_ and one hard-coded drift).  strides[b] belongs to poses[b]: pose b's products are
 * exactly what fpe_plan returns for that pose ALONE with params->stepLength = strides[b].step_length and params->lateralDrift =
 * strides[b].lateral_drift, every other parameter shared by the batch; its summary, score and rank are likewise what fpe_plan_rank
 * computes for it with those two values.  The constants follow the reference's typing (derive_constants): step = double(s),
 * stepHalf = double(s / 2) and stepQuarter = double(s / 4) with the divisions in float, drift = d — so this covers pose_status
 * (the first cycle's gate adds `step`), the walk gait (stepQuarter) and the ranking's cog_speed_* (their first current feet are
 * stance - stepHalf).  Nothing the host proves about windows, discs, rings or rectangles depends on either value.
 * strides == NULL is fpe_plan / fpe_plan_rank itself: the same checks, the same kernel as today.
 * Kernels: every plan kernel family has a stride instantiation (fpe_describe_plan_strides names the one a stride call launches,
 * "... stride (...)").  There is no stride form of the 3x3-only 8-lane variants: a stride call on such a configuration runs the
 * generic variant, which computes the same products (what "no_mid_variant" 1 runs), more slowly.  The direct kernels have stride
 * forms at the automatic group sizes (8 lanes per leg, one wavefront per pose = "plan_group" 65); a stride call under a forced
 * "plan_group" of 4, 16 or 64 returns FPE_E_UNSUPPORTED.
 * Refusals, host forms: a non-finite step_length or lateral_drift, or reserved != 0, in ANY element returns FPE_E_INVALID_ARG and
 * writes nothing; any finite value is taken, zero and negative included (what validate_params takes for the two parameters).
 * Device forms cannot look at the values.  A non-finite stride takes the path a non-finite pose position takes today — every leg
 * centre derived from it fails centre_usable ahead of any index: a non-finite step_length gives, in every cycle, nominal records
 * with valid 0, source 2, row = col = -1 and the non-finite centre as x / y, centroid records of code 6 (zeros, row = col = -1),
 * default_next holding the non-finite positions with z = h, cycle_ok 0, and pose_status FPE_POSE_OPT_SUBMAP_FAILED; a non-finite
 * lateral_drift leaves cycle 0 (which has seen no drift yet) and pose_status as planned and gives every later cycle those records.
 * reserved is not read by the kernels.
 * Out of scope, unchanged: the opt track (fpe_plan_opt*), the service calls (fpe_plan_service*), fpe_multi_* (and dist.py) — all of
 * them keep the one stride of fpe_params — and stride forms of the 3x3-only ("MID") kernels (above). */
typedef struct fpe_stride {   /* 16 bytes; element b belongs to poses[b] */
    float   step_length;      /* replaces fpe_params.stepLength for this pose */
    int32_t reserved;         /* 0 */
    double  lateral_drift;    /* replaces fpe_params.lateralDrift for this pose */
} fpe_stride;
/* fpe_plan / fpe_plan_device with one stride per pose (host array / device array of B elements, or NULL). */
int fpe_plan_strides(fpe_handle h, const fpe_params* params, const fpe_pose* poses, const fpe_stride* strides, int32_t B,
                     int32_t n_cycles, const fpe_plan_out* out);
int fpe_plan_strides_device(fpe_handle h, const fpe_params* params, const fpe_pose* d_poses, const fpe_stride* d_strides, int32_t B,
                            int32_t n_cycles, const fpe_plan_out* d_out, void* stream);
/* fpe_plan_rank / fpe_plan_rank_device with one stride per pose: the candidates of ONE ranking may differ in stride. */
int fpe_plan_rank_strides(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_pose* poses,
                          const fpe_stride* strides, int32_t B, int32_t n_cycles, int32_t K, const fpe_rank_out* out);
int fpe_plan_rank_strides_device(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_pose* d_poses,
                                 const fpe_stride* d_strides, int32_t B, int32_t n_cycles, int32_t K,
                                 const fpe_plan_out* d_full /* may be NULL */, const fpe_rank_out* d_out, void* stream);
/* fpe_describe_plan for the kernel a stride call (strides != NULL) launches on the current map. */
int fpe_describe_plan_strides(fpe_handle h, const fpe_params* params, char* buf, int32_t n);

/* ---- resumable plans: the chain's state across the call boundary, in both directions ---------------------------------------------
 * BUILD-DEFINED (the reference's request carries the four *_current_foothold points, GlobalFootholdPlan.srv:1-4, and its handler
 * never reads them: every plan starts from setFirstGait, cpp:2679-2699).  The state of a pose's chain BETWEEN two gait cycles is the
 * committed feet x / y of the three tracks, the running ajustedPose_[1] and the cycle index — fpe_plan_state.  fpe_plan_resume*
 * returns it behind the last cycle (state_out) and starts a plan from it (state_in) instead of from the nominal stance: replan the
 * remaining cycles on a new map snapshot, branch a plan with several strides, plan a long horizon in segments.
 * The contract:
 *  - Concatenation.  For any pose, any n and any 0 < k < n: k cycles with state_out, then n - k cycles with that state as state_in,
 *    give — concatenated per pose — nominal, centroid, default_next, cycle_ok, selected and selected_packed byte for byte as ONE call
 *    of n cycles returns them, gait_cycle_id included (a resumed record carries state.cycle + g); the second call's state_out equals
 *    the n-cycle call's state_out.
 *  - Indexing.  Inside a call, record (b, g, leg) sits at ((b * n_cycles) + g) * 4 + leg with g LOCAL to the call.
 *  - Start from the poses.  state_in == NULL: the call is fpe_plan_strides plus the state (all eight products).
 *    fpe_plan_state_from_pose returns what such a call starts from: stance - double(step / 2) in all three tracks (the division in
 *    float), adjusted_y 0, cycle 0.
 *  - What a resumed call reads.  state_in != NULL: of poses[b] the kernels read only position[1] (N.y = initialPose_[1] +
 *    ajustedPose_[1], cpp:2201), gait, the leg radii and the polygon kinds.  (The host forms still check every field of every pose.)
 *  - Refused products.  stance and pose_status are products of a START, not of a continuation: a resumed call (state_in != NULL)
 *    that asks for either returns FPE_E_INVALID_ARG and writes nothing.
 *  - Failed cycles.  A cycle that fails commits nothing, the walk gait commits per phase — as in fpe_plan; adjusted_y and cycle
 *    advance all the same.
 *  - Strides.  strides == NULL: every pose uses the stride of `params`.  The stride may change from one segment to the next.
 *  - Aliasing.  state_out may be the same array as state_in: a pose reads its element in its prologue and writes it behind its last
 *    cycle.
 *  - Refusals, host forms: a non-finite value, reserved != 0, cycle < 0 or cycle + n_cycles > 255 in ANY element, before anything is
 *    queued; 1 <= n_cycles <= 255 (FPE_E_INVALID_ARG; nothing is written).
 *  - Non-finite states, device forms (which cannot look at the values): a state with ANY non-finite foot coordinate or a non-finite
 *    adjusted_y is treated as WHOLLY non-finite — the prologue replaces every feet[..][..][0] with NaN before the first cycle.  The
 *    pose then takes the path a non-finite pose position takes: every leg centre fails centre_usable ahead of any index, and every
 *    cycle holds the records listed above for a non-finite step_length; its state_out holds NaN x in every track.  (No half-finite
 *    state reaches a kernel.)
 *  - cycle past 255 in a device call wraps in the uint8 gait_cycle_id of the records; state_out.cycle itself does not wrap.
 * Kernels: a resume instantiation beside every stride instantiation (fpe_describe_plan_resume: "... resume (...)"); as for strides
 * there is no 3x3-only form, and a forced "plan_group" of 4, 16 or 64 returns FPE_E_UNSUPPORTED.  A call with neither state runs
 * exactly what fpe_plan_strides runs.
 * Out of scope: fpe_plan_rank* (the cog-speed KPI's first current feet are a separate question; resumed segments are scored and
 * pruned on the device by fpe_plan_beam*, below, whose score has no cog-speed term), the opt track, the service calls,
 * fpe_multi_* / dist.py, and z in the state (getDefaultFootholdNext overwrites it with 0, and no track's recurrence reads it). */
typedef struct fpe_plan_state {      /* 208 bytes; element b belongs to poses[b] */
    double  feet[3][4][2];  /* [track: 0 default, 1 centroid, 2 nominal][leg: RF,RH,LH,LF][x, y]: the three tracks'
                               *_currentPosition_ members between two gait cycles (cpp:562-588, 1338-1341, 1413-1416, 1480-1483) */
    double  adjusted_y;     /* ajustedPose_[1] (cpp:759, 1578): the running sum, not cycle * drift */
    int32_t cycle;          /* gait cycles planned so far = gait_cycle_id of the next one */
    int32_t reserved;       /* 0 */
} fpe_plan_state;
/* Host arrays; synchronous.  strides, state_in and state_out may each be NULL. */
int fpe_plan_resume(fpe_handle h, const fpe_params* params, const fpe_pose* poses, const fpe_stride* strides,
                    const fpe_plan_state* state_in, int32_t B, int32_t n_cycles, const fpe_plan_out* out, fpe_plan_state* state_out);
/* Device arrays; asynchronous on `stream`, snapshot semantics of fpe_plan_device. */
int fpe_plan_resume_device(fpe_handle h, const fpe_params* params, const fpe_pose* d_poses, const fpe_stride* d_strides,
                           const fpe_plan_state* d_state_in, int32_t B, int32_t n_cycles, const fpe_plan_out* d_out,
                           fpe_plan_state* d_state_out, void* stream);
/* What a call with state_in == NULL starts pose `pose` from (stride NULL: the stride of params).  Host arithmetic only; no engine. */
int fpe_plan_state_from_pose(const fpe_params* params, const fpe_pose* pose, const fpe_stride* stride, fpe_plan_state* out);
/* A state whose three tracks all stand on the given feet ([leg: RF,RH,LH,LF][x, y]) — the seam for the request's four
 * *_current_foothold points.  Finite values and 0 <= cycle <= 254, else FPE_E_INVALID_ARG.  Host arithmetic only; no engine. */
int fpe_plan_state_from_feet(const double feet_xy[4][2], double adjusted_y, int32_t cycle, fpe_plan_state* out);
/* fpe_describe_plan for the kernel a resume call (either state given) launches on the current map. */
int fpe_describe_plan_resume(fpe_handle h, const fpe_params* params, char* buf, int32_t n);

/* ---- beam search over stride options on the device, on resumable plans ---------------------------------------------------------
 * BUILD-DEFINED (the reference has one stride, and a failing cycle of it commits nothing: the next cycle retries from the same
 * feet).  The planner chooses its strides: S segments of k gait cycles; in every segment each kept plan of a root pose is continued
 * with each of the M stride options, the continuations are scored, and the best W per root are kept.  Expand, score, prune,
 * remember and trace back run on the device, on one stream, with no host synchronisation between segments; the chain arithmetic is
 * fpe_plan_resume's (one resume launch per segment, one map snapshot for the whole beam) and nothing here adds search arithmetic.
 * Every root pose b has its own beam; roots never compete with one another.
 *  - Parents of segment 0.  One per root: state_in[b], or "start from the pose" when state_in == NULL; penalty +0.0; n_{-1} = 1.
 *  - Candidates of segment s.  Parent slot p < n_{s-1} and option m < M give candidate c = p * M + m: k cycles of fpe_plan_resume
 *    for poses[b] with the stride options[m] from the parent's state.  In segment 0 with state_in == NULL it is exactly what
 *    fpe_plan_strides computes for that pose and stride (the half-step shift of the start depends on the option).
 *  - Segment penalty.  q = w_fail*(k - committed) + w_spiral*n_source[1] + w_none*(n_source[2] + n_source[3]) +
 *    w_deviation*deviation_sq_sum, with committed, n_source and deviation_sq_sum as fpe_pose_summary defines them over the segment's
 *    k cycles: each product first, the four terms added left to right in f64, no contraction.  P_c = P_parent + q.
 *  - Progress.  cx = ((x_RF + x_RH) + (x_LH + x_LF)) * 0.25 over the NOMINAL track (feet[2]) of the candidate's state behind the
 *    segment.  Candidates of one root are compared only among themselves, so the absolute cx needs no baseline.
 *  - Score.  t = w_progress * cx, then score = P_c - t (two operations, no fused multiply-add); -0.0 is stored as +0.0.  There is no
 *    cog-speed term (fpe_plan_rank's KPI assumes a start from the stance), so walk-gait roots are ordinary.
 *  - Order and survivors.  (class, score, c) ascending; class 1 = non-finite score, ordered by c alone; equal scores (IEEE ==) fall
 *    to c.  n_s = min(W, n_{s-1} * M), the same for every root; the survivors fill slots 0 .. n_s - 1 in order.
 *  - Outputs for live slot (b, w), w < n_{S-1}, best first, at element b * W + w: score and penalty of the last segment; path[s],
 *    the option taken in segment s along the slot's ancestry; state, behind the last cycle; products, the ancestry's segments
 *    concatenated — record (g, leg) of the slot's S * k cycles sits where ONE fpe_plan_resume call of S * k cycles for B * W poses
 *    would put it, gait_cycle_id = state.cycle + g.  n_live[b] = n_{S-1}.  Dead slots (w >= n_live) are NOT WRITTEN, in every output
 *    array.  No atomics: every byte is a function of the inputs alone.
 *  - Replay.  For any live slot, S successive fpe_plan_resume calls of k cycles for poses[b] with the stride options[path[s]] and
 *    the state carried over give the slot's products (concatenated) and its state byte for byte.
 *  - Refusals (FPE_E_INVALID_ARG; nothing written or queued): M outside 1..FPE_BEAM_MAX_OPTIONS, width outside
 *    1..FPE_BEAM_MAX_WIDTH, segments or cycles_per_segment < 1, segments * cycles_per_segment > 255, B < 1, B * width * M >
 *    FPE_BEAM_MAX_CHAINS, reserved != 0, a non-finite weight, path == NULL, stance or pose_status requested (products of a start,
 *    as for a resumed plan).  The host form also refuses what fpe_plan_resume refuses for poses, options and states, with cycle +
 *    segments * cycles_per_segment > 255 in place of its cycle bound.  A forced "plan_group" of 4, 16 or 64 returns
 *    FPE_E_UNSUPPORTED (no resume kernel exists there); the map-size bound of selected_packed applies when that product is requested.
 *  - Device form.  It cannot look at the values: a non-finite option or state takes the resume kernels' documented path.  A chain
 *    that STARTS from a non-finite value — a non-finite state, or a non-finite step length from the poses (the start is stance -
 *    step / 2) — has NaN x in every track, which gives a NaN cx: the candidate is class 1, and so is every descendant.  A non-finite
 *    step length on a finite parent state fails every cycle and commits nothing: the candidate keeps its parent's feet, so it is
 *    class 0 with k failed cycles in its penalty.
 * The swing, trunk and margin checks in the pruning: the checked beam (fpe_plan_beam_checked*, behind the checked ranking).
 * Out of scope: a global beam across roots, deduplication of equal states, the opt track, the service calls, fpe_multi_* / dist.py. */
#define FPE_BEAM_MAX_OPTIONS 16
#define FPE_BEAM_MAX_WIDTH   64
#define FPE_BEAM_MAX_CHAINS  (1 << 20)   /* B * width * n_options */
typedef struct fpe_beam_params {          /* 56 bytes */
    int32_t segments;            /* S >= 1 */
    int32_t cycles_per_segment;  /* k >= 1; S * k <= 255 */
    int32_t width;               /* W, 1..FPE_BEAM_MAX_WIDTH: beam entries kept PER ROOT pose */
    int32_t reserved;            /* 0 */
    double  w_fail, w_spiral, w_none, w_deviation, w_progress;   /* all finite */
} fpe_beam_params;
/* build-defined defaults: segments 4, cycles_per_segment 2, width 8; w_fail 100, w_spiral 1, w_none 0, w_deviation 10, w_progress 100 */
int fpe_beam_params_defaults(fpe_beam_params* out);
typedef struct fpe_beam_out {             /* 104 bytes */
    int32_t* n_live;        /* [B] live entries of each root's final beam, or NULL */
    double*  score;         /* [B * W] or NULL */
    double*  penalty;       /* [B * W] or NULL */
    uint8_t* path;          /* [B * W * S] option index taken in each segment — required */
    fpe_plan_state* state;  /* [B * W] state behind the last cycle, or NULL */
    fpe_plan_out products;  /* shapes of fpe_plan_out with B -> B * W and n_cycles -> S * k; any pointer may be NULL;
                               stance and pose_status must be NULL (FPE_E_INVALID_ARG), as for a resumed plan */
} fpe_beam_out;
/* Host arrays; synchronous.  beam NULL = fpe_beam_params_defaults; state_in may be NULL; options: M elements. */
int fpe_plan_beam(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, const fpe_pose* poses,
                  const fpe_plan_state* state_in, int32_t B, const fpe_stride* options, int32_t M, const fpe_beam_out* out);
/* Device arrays (every non-NULL pointer of d_out too); asynchronous on `stream`, snapshot semantics of fpe_plan_device.  The
 * candidates, keys and the history live in one stream-ordered scratch block. */
int fpe_plan_beam_device(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, const fpe_pose* d_poses,
                         const fpe_plan_state* d_state_in, int32_t B, const fpe_stride* d_options, int32_t M,
                         const fpe_beam_out* d_out, void* stream);

/* ---- the dense maps as grid_map message layers: the inverse of fpe_upload_map's ingest ----------------------------------
 * BUILD-DEFINED (the reference publishes none of these layers).  One call runs the dense families whose layers are requested —
 * fpe_foothold_map, fpe_foothold_snap, fpe_centroid_map with the same params, roi, radius and polygon; only the products
 * those layers need — and writes every requested layer as rows * cols floats of the WHOLE map in the layout of the message
 * being filled: canonical cell (i, j) goes to buffer cell bi = (i + start_index[0]) mod rows, bj = (j + start_index[1]) mod
 * cols, which is element bi + bj * rows of a column-major buffer (storage_order 0) and bi * cols + bj of a row-major one
 * (fpe_map_desc's mapping, inverted).  Inside roi the value is the layer's float of the table below, computed from exactly
 * what the dense call returns; outside roi it is the quiet NaN 0x7FC00000 (grid_map's "no data").  Every call writes every
 * cell of every requested destination; a refused call writes nothing.  Refusals: FPE_E_INVALID_ARG for a null handle, params
 * or request, n_layers out of range, an unknown or duplicated id, a null dst, a start index outside the map, a storage order
 * other than 0 or 1, a bad roi; FPE_E_NO_MAP; and every refusal of the dense calls of the families requested (a bad polygon
 * kind is refused only when a snap layer is requested).  Snapshot semantics, literal_discs and pinned destinations behave as in
 * fpe_foothold_map: the host form is synchronous, the device form asynchronous on `stream`. */
/* layer ids; the float a layer holds for canonical cell (i, j) inside the region */
#define FPE_LAYER_FOOTHOLD_FLAGS  0  /* (float) fpe_foothold_map flags byte, 0..7            */
#define FPE_LAYER_FOOTHOLD_HEIGHT 1  /* fpe_foothold_map height, bit for bit                 */
#define FPE_LAYER_SNAP_DI         2  /* (float) fpe_foothold_snap offset[0]                  */
#define FPE_LAYER_SNAP_DJ         3  /* (float) offset[1]                                    */
#define FPE_LAYER_SNAP_SOURCE     4  /* (float) source                                       */
#define FPE_LAYER_SNAP_Z          5  /* z, bit for bit                                       */
#define FPE_LAYER_CENTROID_CODE   6  /* (float) fpe_centroid_map code                        */
#define FPE_LAYER_CENTROID_DI     7  /* (float) fpe_centroid_map offset[0]                   */
#define FPE_LAYER_CENTROID_DJ     8  /* (float) offset[1]                                    */
#define FPE_LAYER_CENTROID_Z      9  /* z, bit for bit                                       */
#define FPE_LAYER_COUNT          10

typedef struct fpe_layer_layout {      /* the DESTINATION buffers' layout: that of the message being filled */
    int32_t start_index[2];            /* 0 <= start_index[k] < size[k] */
    int32_t storage_order;             /* 0 column-major (grid_map_msgs), 1 row-major — as fpe_map_desc */
    int32_t reserved;                  /* 0 */
} fpe_layer_layout;                    /* NULL layout = canonical: start (0,0), row-major */

typedef struct fpe_layer_request {
    int32_t n_layers;                  /* 1..FPE_LAYER_COUNT */
    int32_t layer[FPE_LAYER_COUNT];    /* FPE_LAYER_* ids, no duplicates */
    float*  dst[FPE_LAYER_COUNT];      /* dst[k]: rows*cols floats of the WHOLE map for layer[k]; non-NULL */
    float   snap_search_radius;        /* as fpe_foothold_snap (<= 0: params->searchRadius) */
    int32_t snap_polygon_kind;         /* as fpe_foothold_snap */
    float   centroid_search_radius;    /* as fpe_centroid_map */
    int32_t reserved;
} fpe_layer_request;

int fpe_export_layers(fpe_handle h, const fpe_params* params, const int32_t roi[4], const fpe_layer_layout* layout,
                      const fpe_layer_request* request);
int fpe_export_layers_device(fpe_handle h, const fpe_params* params, const int32_t roi[4], const fpe_layer_layout* layout,
                             const fpe_layer_request* d_request /* dst = DEVICE pointers */, void* stream);

/* ---- swing checks: each planned step against the elevation layer ------------------------------------------------------------------
 * BUILD-DEFINED (the reference reads the elevation layer for getFootholdMeanHeight alone and never looks at the ground between two
 * successive footholds of a leg).  A SEGMENT runs from A = (ax, ay, az) to B = (bx, by, bz), all doubles, with a radius
 * r = double(float radius).  On the snapshot current at entry, with MapGeom g (csrc/fpe_gridmath.hpp), a cell (i, j), 0 <= i < rows,
 * 0 <= j < cols, belongs to the segment's CAPSULE iff, in f64, in exactly this order, without contraction:
 *     px = cell_pos(g.baseX, g.res, i);  py = cell_pos(g.baseY, g.res, j)
 *     dx = bx - ax;  dy = by - ay;  L2 = dx*dx + dy*dy
 *     t  = L2 > 0 ? ((px-ax)*dx + (py-ay)*dy) / L2 : 0;   t = t < 0 ? 0 : (t > 1 ? 1 : t)
 *     ex = px - (ax + t*dx);  ey = py - (ay + t*dy)
 *     member  <=>  ex*ex + ey*ey <= r*r
 * A member with elevation e (f32) is KNOWN iff isfinite(e) && e < 10.0f — the cut of getFootholdMeanHeight (cpp:2533), so the check and
 * the plan's z agree on which cells count.  A known member has lift_c = double(e) - (az + t*(bz - az)): its height above the straight
 * line between the two foot heights.  Every quantity of a record is order-free — a count, a maximum, or an argmax with a stated tie
 * rule — so its value does not depend on how the device splits the cells:
 *   lift           the maximum lift_c over the known members: what a swing must clear above the chord.  +0.0 when there is none.
 *                  Maxima are taken in IEEE-754 totalOrder (+0.0 ranks above -0.0; no value is NaN), so the bits are defined too;
 *   row, col       the known member attaining `lift`; among several the lowest row, then the lowest column.  (-1, -1) when none;
 *   max_elevation  the maximum e over the known members (totalOrder); 0 when there is none;
 *   n_cells        members (inside the map);  n_unknown: members that are not known;
 *   rise           bz - az;
 *   length_sq      L2 — the square, so that nothing rests on a device square root;
 *   flags          FPE_SWING_* bits, below.
 * Radius: query.radius <= 0 means limits.radius, and that, if <= 0, params.footRadius.
 * Limits: a NULL `limits` is fpe_swing_limits_defaults — the three limits +infinity (no OVER bit is ever set), radius 0.
 * Refusals.  Every form returns FPE_E_INVALID_ARG for a null argument, n or B < 1, n_cycles outside 1..255, limits.reserved != 0, a NaN
 * limit, or a default radius (limits.radius, else params.footRadius) that is not finite or above FPE_SWING_MAX_RADIUS.  The host forms
 * also refuse — nothing is queued or written — a query with reserved != 0, a non-finite coordinate or radius, |coordinate| > 1e6, or a
 * radius above FPE_SWING_MAX_RADIUS, and fpe_swing_plan what fpe_plan refuses.  The device forms cannot look at the values: such a
 * segment (reserved is not read) gives a record with flags = FPE_SWING_REFUSED and every other field zero.  FPE_E_UNSUPPORTED on a
 * map with a resolution below 1e-4 m or a cell farther than 2e6 m from the origin on either axis: the kernels' cell enumeration is
 * proven a superset of the members for the rest (csrc/fpe_swing.hpp).
 * The plan-bound segments are what a consumer of the GlobalFootholds message executes.  With the products nominal [B, n, 4], cycle_ok
 * [B, n] and the start feet [B, 4, 3] (x, y, z of RF, RH, LH, LF), record (b, g, leg) at ((b * n_cycles) + g) * 4 + leg:
 *   - describes a segment iff cycle_ok[b, g] != 0;  B = nominal[b, g, leg] as (x, y, double(z));
 *   - A = the same leg's nominal record of the latest g' < g with cycle_ok[b, g'] != 0, or start_feet[b, leg] when there is none;
 *   - equals, bit for bit, the record the open-loop form returns for the query {A, B, radius 0}, with foot_id = leg and
 *     gait_cycle_id = g filled in (the open-loop form leaves both 0);
 *   - of a cycle that did not commit: all zero but foot_id and gait_cycle_id.
 * The start feet default to the plan's `stance` product.  stance carries the POSE's z, not a terrain height (RF/RH/LH/LF_initialPosition_,
 * cpp:350-378): the first swing's rise and lift are then relative to the body height given in the pose.  A caller that knows where the feet
 * stand — a resumed plan, heights read from the map — hands in feet of its own.
 * The per-pose summary covers the records of the pose that describe a segment, whatever else their flags say: max_lift (totalOrder),
 * max_abs_rise = max fabs(rise), max_length_sq, each 0 when the pose has no segment; n_segments; n_over: segments with any OVER bit;
 * n_unknown: segments with UNKNOWN, EMPTY or OFF_MAP; first_over_cycle: the lowest g of a segment with an OVER bit, 255 when none.
 * No atomics anywhere: every byte is a function of the inputs alone.  A swing term in the ranking: the checked ranking below
 * (fpe_plan_rank_checked*); in the beam's pruning: the checked beam (fpe_plan_beam_checked*).  Out of scope: fpe_multi_*, the
 * service calls, the opt and centroid tracks' footholds, any trajectory shape beyond the lift above the chord. */
#define FPE_SWING_SEGMENT     1u   /* the record describes a segment */
#define FPE_SWING_OFF_MAP     2u   /* A or B fails checkIfPositionWithinMap (within_axis on either axis) */
#define FPE_SWING_EMPTY       4u   /* n_cells == 0 */
#define FPE_SWING_UNKNOWN     8u   /* n_unknown > 0 */
#define FPE_SWING_OVER_LIFT   16u  /* lift > limits.max_lift */
#define FPE_SWING_OVER_RISE   32u  /* fabs(rise) > limits.max_rise */
#define FPE_SWING_OVER_LENGTH 64u  /* length_sq > limits.max_length * limits.max_length */
#define FPE_SWING_REFUSED     128u /* device forms: a segment the host forms refuse; every other field zero, SEGMENT not set */
#define FPE_SWING_MAX_RADIUS  0.5f
typedef struct fpe_swing_query {      /* 56 bytes */
    double  a[3], b[3];    /* A and B: x, y, z */
    float   radius;        /* <= 0: limits.radius, else params.footRadius */
    int32_t reserved;      /* 0 */
} fpe_swing_query;
typedef struct fpe_swing_limits {     /* 32 bytes */
    double  max_lift, max_rise, max_length;   /* not NaN; +infinity: no limit */
    float   radius;        /* the capsule radius of queries that give none; <= 0: params.footRadius */
    int32_t reserved;      /* 0 */
} fpe_swing_limits;
typedef struct fpe_swing_record {     /* 48 bytes */
    double  lift, rise, length_sq;
    float   max_elevation;
    int32_t n_cells, n_unknown;
    int32_t row, col;
    uint8_t flags;         /* FPE_SWING_* */
    uint8_t foot_id;       /* plan-bound: 0 RF, 1 RH, 2 LH, 3 LF; open-loop: 0 */
    uint8_t gait_cycle_id; /* plan-bound: g; open-loop: 0 */
    uint8_t pad;
} fpe_swing_record;
typedef struct fpe_swing_summary {    /* 40 bytes; element b belongs to pose b */
    double  max_lift, max_abs_rise, max_length_sq;
    int32_t n_segments, n_over, n_unknown;
    uint8_t first_over_cycle;  /* 255: none */
    uint8_t pad[3];
} fpe_swing_summary;
typedef struct fpe_swing_out {        /* 16 bytes; either pointer may be NULL */
    fpe_swing_record*  records;  /* [B * n_cycles * 4] */
    fpe_swing_summary* summary;  /* [B] */
} fpe_swing_out;
int fpe_swing_limits_defaults(fpe_swing_limits* out);
/* Open-loop: n arbitrary segments.  Host arrays, synchronous / device arrays, asynchronous on `stream`. */
int fpe_swing_segments(fpe_handle h, const fpe_params* params, const fpe_swing_limits* limits, const fpe_swing_query* queries, int32_t n,
                       fpe_swing_record* out);
int fpe_swing_segments_device(fpe_handle h, const fpe_params* params, const fpe_swing_limits* limits, const fpe_swing_query* d_queries,
                              int32_t n, fpe_swing_record* d_out, void* stream);
/* Plan-bound, device arrays: reads d_products->nominal and ->cycle_ok (both required) as a plan call on `stream` left them, and
 * ->stance when d_start_feet (B * 4 * 3 doubles) is NULL; `d_products` and `d_out` themselves are host structs of device pointers.
 * Asynchronous on `stream`, behind whatever filled the products there. */
int fpe_swing_plan_device(fpe_handle h, const fpe_params* params, const fpe_swing_limits* limits, const fpe_plan_out* d_products,
                          const double* d_start_feet, int32_t B, int32_t n_cycles, const fpe_swing_out* d_out, void* stream);
/* Plan and check in one call, host arrays, synchronous: plans exactly as fpe_plan (strides NULL) or fpe_plan_strides would, checks the
 * plan on the same stream with no host synchronisation in between, on ONE snapshot, and returns the requested products (NULL: none)
 * and the swing outputs.  The start feet are the plan's stance. */
int fpe_swing_plan(fpe_handle h, const fpe_params* params, const fpe_swing_limits* limits, const fpe_pose* poses,
                   const fpe_stride* strides, int32_t B, int32_t n_cycles, const fpe_plan_out* products, const fpe_swing_out* out);

/* ---- trunk checks: each planned stance's body box against the elevation layer ------------------------------------------------------
 * BUILD-DEFINED (the reference never looks at the ground under the body: a plan whose footholds and swings all pass can still put the
 * belly on a kerb, a stair nose or a block the feet straddle).  A STANCE is four feet f[leg] = (x, y, z), all doubles, in the order
 * RF, RH, LH, LF — in the reference's stance (cpp:350-378) the front feet are RF and LF, and the left feet LH and LF have the larger
 * y — and a box of half extents hx, hy, each double(float).  All arithmetic is f64, in exactly this order, without contraction:
 *     cx  = ((x0 + x1) + (x2 + x3)) * 0.25;   cy, zm likewise from y and z
 *     dxf = ((x0 + x3) - (x1 + x2)) * 0.5;    dzf = ((z0 + z3) - (z1 + z2)) * 0.5      front minus hind
 *     dyl = ((y2 + y3) - (y0 + y1)) * 0.5;    dzl = ((z2 + z3) - (z0 + z1)) * 0.5      left minus right
 *     slope_x = dxf > 0 ? dzf / dxf : 0;      slope_y = dyl > 0 ? dzl / dyl : 0
 *     base_z  = zm + limits.ride_height
 * On the snapshot current at entry, with MapGeom g (csrc/fpe_gridmath.hpp), cell (i, j), 0 <= i < rows, 0 <= j < cols, is a MEMBER iff
 *     px = cell_pos(g.baseX, g.res, i);  py = cell_pos(g.baseY, g.res, j);      fabs(px - cx) <= hx  &&  fabs(py - cy) <= hy
 * so the members are an index rectangle, decided per row and per column.  A member with elevation e (f32) is KNOWN iff isfinite(e) &&
 * e < 10.0f — the cut of getFootholdMeanHeight (cpp:2533) and of the swing check — and a known member has
 *     gap_c = (base_z + (slope_x * (px - cx) + slope_y * (py - cy))) - double(e)
 * the height of the body plane through the feet, lifted by ride_height, above the ground of that cell.  Every quantity of a record is
 * order-free — a count, an extremum, or an argmin with a stated tie rule:
 *   clearance      the minimum gap_c over the known members, taken in IEEE-754 totalOrder (-0.0 ranks below +0.0; nothing is NaN: see
 *                  the slope bound below), so the bits are defined and clearance is the gap_c of the cell the record names.  +infinity
 *                  when there is no known member;
 *   row, col       the known member attaining it; among several the lowest row, then the lowest column.  (-1, -1) when there is none;
 *   slope_x, slope_y, base_z   as derived above: what a controller sets body pitch, roll and height from;
 *   max_elevation  the totalOrder maximum of e over the known members; 0 when there is none;
 *   n_cells        members (inside the map);  n_unknown: members that are not known;
 *   flags          FPE_TRUNK_* bits, below.
 * Half extents: query.half_length / half_width <= 0 means the limits' value, and that, if <= 0, 0.5 * double(params.length) /
 * 0.5 * double(params.width).  Limits: a NULL `limits` is fpe_trunk_limits_defaults — min_clearance -infinity, both slope limits
 * +infinity (no UNDER / OVER bit is ever set), ride_height 0, both half extents 0.
 * Refusals.  Every form returns FPE_E_INVALID_ARG for a null argument, n or B < 1, n_cycles outside 1..255, a limits.reserved word
 * that is not 0, a NaN limit, a ride_height that is not finite or beyond +-1e6, or a default half extent (the limits', else half the
 * params') that is not finite, <= 0 or above FPE_TRUNK_MAX_HALF_EXTENT; FPE_E_UNSUPPORTED on the maps the swing check refuses (a
 * resolution below 1e-4 m, a cell farther than 2e6 m from the origin: the kernels' cell enumeration is proven a superset of the
 * members for the rest, csrc/fpe_trunk.hpp) and when the default box exceeds FPE_TRUNK_MAX_CELLS by the f64 expression
 *     (2.0 * hx / g.res + 3.0) * (2.0 * hy / g.res + 3.0) > FPE_TRUNK_MAX_CELLS
 * The host forms also refuse (FPE_E_INVALID_ARG; nothing is queued or written) a stance with a query.reserved word that is not 0, a
 * non-finite coordinate, |coordinate| > 1e6, a half extent that is not finite or above FPE_TRUNK_MAX_HALF_EXTENT, a box over the cell
 * cap by the same expression, or a slope beyond +-FPE_TRUNK_MAX_SLOPE; fpe_trunk_plan refuses what fpe_plan refuses.  The slope
 * bound is what makes "nothing is NaN" true: feet a hair apart give an infinite slope, and infinity times a zero offset is a NaN whose
 * bits differ between machines; within the bound every gap_c is finite.  The device forms cannot look at the values: such a stance
 * (reserved is not read) gives a record with flags = FPE_TRUNK_REFUSED and every other field zero, decided per record in the kernel by
 * the same expressions.
 * The plan-bound stances are the four feet on the ground when cycle g of a plan has landed.  With the products nominal [B, n, 4] and
 * cycle_ok [B, n], record (b, g) at b * n_cycles + g:
 *   - describes a stance iff cycle_ok[b, g] != 0;  its feet are nominal[b, g, leg] as (x, y, double(z)), its half extents the defaults;
 *   - equals, bit for bit, the record the open-loop form returns for that query, with gait_cycle_id = g filled in;
 *   - of a cycle that did not commit: all zero but gait_cycle_id.
 * Successive boxes of one pose overlap by construction — a cycle moves the feet by the step length (0.18 m in the yaml), far below
 * the body length (0.4387 m) — so the ground under the moving trunk is covered from cycle to cycle by the union of the records.  The
 * half-cycle stances of the trot's two diagonal pairs (two feet down, two in the air) are not checked.
 * The per-pose summary runs over the pose's records that describe a stance, whatever else their flags say: min_clearance (totalOrder;
 * +infinity when there is none), max_abs_slope_x / _y = max fabs(slope) (0 when none), n_stances, n_bad: stances with UNDER_CLEARANCE
 * or OVER_SLOPE, n_unknown: stances with UNKNOWN, EMPTY or OFF_MAP, first_bad_cycle: the lowest g of a bad stance, 255 when none.
 * No atomics anywhere: every byte is a function of the inputs alone.  A trunk term in the ranking: the checked ranking below
 * (fpe_plan_rank_checked*); in the beam's pruning: the checked beam (fpe_plan_beam_checked*).  Out of scope: fpe_multi_*, the
 * service calls, the opt and centroid tracks' footholds, yaw (the box is axis-aligned in the map frame, as the reference's stance is), the trot's half-cycle stances, any body shape other
 * than the axis-aligned box. */
#define FPE_TRUNK_STANCE          1u   /* the record describes a stance */
#define FPE_TRUNK_OFF_MAP         2u   /* any of the four corners (cx +- hx, cy +- hy) fails checkIfPositionWithinMap (within_axis) */
#define FPE_TRUNK_EMPTY           4u   /* n_cells == 0 */
#define FPE_TRUNK_UNKNOWN         8u   /* n_unknown > 0 */
#define FPE_TRUNK_UNDER_CLEARANCE 16u  /* clearance < limits.min_clearance */
#define FPE_TRUNK_OVER_SLOPE      32u  /* fabs(slope_x) > limits.max_slope_x || fabs(slope_y) > limits.max_slope_y */
#define FPE_TRUNK_DEGENERATE      64u  /* !(dxf > 0) || !(dyl > 0): the slope of that axis is 0 */
#define FPE_TRUNK_REFUSED         128u /* device forms: a stance the host forms refuse; every other field zero, STANCE not set */
#define FPE_TRUNK_MAX_HALF_EXTENT 1.0f
#define FPE_TRUNK_MAX_CELLS       65536
#define FPE_TRUNK_MAX_SLOPE       1e6
typedef struct fpe_trunk_query {      /* 112 bytes */
    double  feet[4][3];    /* RF, RH, LH, LF: x, y, z */
    float   half_length;   /* hx; <= 0: limits.half_length, else 0.5 * params.length */
    float   half_width;    /* hy; <= 0: limits.half_width, else 0.5 * params.width */
    int32_t reserved[2];   /* 0 */
} fpe_trunk_query;
typedef struct fpe_trunk_limits {     /* 48 bytes */
    double  min_clearance;            /* not NaN; -infinity: no limit */
    double  max_slope_x, max_slope_y; /* not NaN; +infinity: no limit */
    double  ride_height;              /* finite, |ride_height| <= 1e6: the body plane's height above the plane through the feet */
    float   half_length, half_width;  /* the box of stances that give none; <= 0: half of params.length / params.width */
    int32_t reserved[2];              /* 0 */
} fpe_trunk_limits;
typedef struct fpe_trunk_record {     /* 56 bytes */
    double  clearance, slope_x, slope_y, base_z;
    float   max_elevation;
    int32_t n_cells, n_unknown;
    int32_t row, col;
    uint8_t flags;         /* FPE_TRUNK_* */
    uint8_t gait_cycle_id; /* plan-bound: g; open-loop: 0 */
    uint8_t pad[2];
} fpe_trunk_record;
typedef struct fpe_trunk_summary {    /* 40 bytes; element b belongs to pose b */
    double  min_clearance, max_abs_slope_x, max_abs_slope_y;
    int32_t n_stances, n_bad, n_unknown;
    uint8_t first_bad_cycle;  /* 255: none */
    uint8_t pad[3];
} fpe_trunk_summary;
typedef struct fpe_trunk_out {        /* 16 bytes; either pointer may be NULL */
    fpe_trunk_record*  records;  /* [B * n_cycles] */
    fpe_trunk_summary* summary;  /* [B] */
} fpe_trunk_out;
int fpe_trunk_limits_defaults(fpe_trunk_limits* out);
/* Open-loop: n arbitrary stances.  Host arrays, synchronous / device arrays, asynchronous on `stream`. */
int fpe_trunk_stances(fpe_handle h, const fpe_params* params, const fpe_trunk_limits* limits, const fpe_trunk_query* queries, int32_t n,
                      fpe_trunk_record* out);
int fpe_trunk_stances_device(fpe_handle h, const fpe_params* params, const fpe_trunk_limits* limits, const fpe_trunk_query* d_queries,
                             int32_t n, fpe_trunk_record* d_out, void* stream);
/* Plan-bound, device arrays: reads d_products->nominal and ->cycle_ok (both required) as a plan call on `stream` left them;
 * `d_products` and `d_out` themselves are host structs of device pointers.  Asynchronous on `stream`, behind whatever filled the
 * products there. */
int fpe_trunk_plan_device(fpe_handle h, const fpe_params* params, const fpe_trunk_limits* limits, const fpe_plan_out* d_products,
                          int32_t B, int32_t n_cycles, const fpe_trunk_out* d_out, void* stream);
/* Plan and check in one call, host arrays, synchronous: plans exactly as fpe_plan (strides NULL) or fpe_plan_strides would, checks the
 * plan on the same stream with no host synchronisation in between, on ONE snapshot, and returns the requested products (NULL: none)
 * and the trunk outputs. */
int fpe_trunk_plan(fpe_handle h, const fpe_params* params, const fpe_trunk_limits* limits, const fpe_pose* poses,
                   const fpe_stride* strides, int32_t B, int32_t n_cycles, const fpe_plan_out* products, const fpe_trunk_out* out);

/* ---- edge margin: the distance from cells and planned footholds to bad ground ---------------------------------------------------------
 * BUILD-DEFINED (the reference answers yes or no against the foot disc: a foothold whose disc just passes on a stair nose and one in the
 * middle of a tread look alike).  Everything is an integer, computed on the snapshot current at entry from its bit planes; all indices
 * are canonical (i, j).  For the threshold pair (thrDefault, thrCandidate) = (params->defaultFootholdThreshold,
 * params->candidateFootholdThreshold) and the f32 traversability t of a cell, the classes are
 *   FPE_MARGIN_LOW_CANDIDATE  the cell is in the map and  isfinite(t) && t < thrCandidate   (plane C: build_bitmap_kernel's compare)
 *   FPE_MARGIN_LOW_DEFAULT    the cell is in the map and  isfinite(t) && t < thrDefault     (plane Df)
 *   FPE_MARGIN_UNKNOWN        the cell is in the map and  !isfinite(t)                      (plane F clear: NaN, +infinity, -infinity)
 *   FPE_MARGIN_OFF_MAP        i < 0, i >= rows, j < 0 or j >= cols
 * so a -infinity cell is UNKNOWN and belongs to no LOW class (the plane D, which holds the raw compare, is not read).  `classes` is a
 * non-empty subset of the four bits; a cell is BAD iff it belongs to a selected class.
 * Margin of a cell.  reach = mp.reach_cells, 1 <= reach <= FPE_MARGIN_MAX_CELLS.  For ANY integer cell (i, j), in the map or not:
 *   dist_sq   min { di^2 + dj^2 : di^2 + dj^2 <= reach^2 and cell (i + di, j + dj) is BAD };  FPE_MARGIN_NONE when the set is empty;
 *   (di, dj)  the offset attaining it; among several the lowest di, then the lowest dj;  (0, 0) when dist_sq is NONE.
 * No square root, no float: there is no tolerance anywhere.  The metric margin is res * sqrt(dist_sq); only a caller computes it.
 * Limit.  min_margin is a double in metres, finite and >= 0.  With MapGeom g (csrc/fpe_gridmath.hpp) and res2 = g.res * g.res formed
 * once, in f64, a record is UNDER iff
 *     dist_sq != FPE_MARGIN_NONE  &&  double(dist_sq) * res2 < min_margin * min_margin
 * so min_margin = 0 sets no bit.  A limit the reach cannot decide is refused with FPE_E_UNSUPPORTED:
 *     min_margin * min_margin > double(reach * reach) * res2
 * Records.  A record of cell (row, col): dist_sq, di, dj as above and flags FOOTHOLD | CENTRE_OFF_MAP (the cell itself is not in the
 * map) | NO_BAD (dist_sq is NONE) | UNDER.  A cell with row < -FPE_PACKED_BIAS, row >= rows + FPE_PACKED_BIAS, or the same for col (a
 * default hit carries getIndex(centre), up to a foot radius outside the map; nothing the planner produces lies farther out) is refused:
 * the host forms return FPE_E_INVALID_ARG and write nothing; the device forms cannot look at the values and give a record with
 * flags = FPE_MARGIN_REFUSED and every other field zero (the plan-bound form: but the two ids), decided by the same expression.
 * Forms.  Dense (fpe_margin_map*): dist_sq and / or nearest = (di, dj) for every cell of a region, roi as fpe_foothold_map.  Open-loop
 * (fpe_margin_cells*): n arbitrary cells; foot_id and gait_cycle_id are 0.  Plan-bound (fpe_margin_plan_device): reads
 * d_products->nominal [B, n_cycles, 4] (required) only; record (b, g, leg) at (b * n_cycles + g) * 4 + leg describes a foothold iff
 * nominal[b, g, leg].valid != 0, its cell is that record's (row, col), and it equals, bit for bit, the open-loop record of that cell
 * with foot_id = leg and gait_cycle_id = g filled in; the record of an invalid foothold is all zero but those two ids.  Note that the
 * margin is that of the record's CELL: up to half a cell off the continuous centre of a default hit.
 * The per-pose summary runs over the pose's records with FOOTHOLD set (a REFUSED record has none): min_dist_sq, NONE taking part as
 * 65535 (65535 when there is no foothold), min_cycle / min_leg the lowest (g, leg) attaining it (255, 255 without a foothold),
 * n_footholds, n_under (UNDER), n_off_map (CENTRE_OFF_MAP), first_under_cycle the lowest g of an UNDER record (255: none).
 * Conventions as fpe_trunk_*: host forms are synchronous; device forms are asynchronous on `stream` and see the snapshot current at
 * entry (the pair's bit planes are built on first use, on that stream).  A NULL `mp` is fpe_margin_params_defaults: classes
 * LOW_CANDIDATE | UNKNOWN | OFF_MAP, reach 8, min_margin 0.
 * Refusals (a refused call writes nothing).  FPE_E_INVALID_ARG: a null argument, n or B < 1, n_cycles outside 1..255 (or
 * B * n_cycles * 4 > 2^30), classes outside 1..15, reach_cells outside 1..FPE_MARGIN_MAX_CELLS, a reserved word that is not 0, a
 * min_margin that is NaN, infinite or negative, a bad roi, both dense outputs NULL, both plan-bound outputs NULL.  FPE_E_NO_MAP.
 * FPE_E_UNSUPPORTED: the undecidable limit above.  fpe_margin_plan also refuses what fpe_plan refuses.
 * No atomics anywhere: every byte is a function of the inputs alone.  A margin term in the ranking: the checked ranking below
 * (fpe_plan_rank_checked*); in the beam's pruning: the checked beam (fpe_plan_beam_checked*).  Out of scope:
 * a margin layer in fpe_export_layers (its request struct has fixed arrays: a new layer would change the ABI); fpe_multi_*, the service
 * calls, the opt and centroid tracks; sub-cell positions (see the note above); reaches beyond FPE_MARGIN_MAX_CELLS cells. */
#define FPE_MARGIN_LOW_CANDIDATE 1u
#define FPE_MARGIN_LOW_DEFAULT   2u
#define FPE_MARGIN_UNKNOWN       4u
#define FPE_MARGIN_OFF_MAP       8u
#define FPE_MARGIN_MAX_CELLS     31
#define FPE_MARGIN_NONE          65535u
#define FPE_MARGIN_FOOTHOLD       1u   /* the record describes a foothold; open-loop records always set it */
#define FPE_MARGIN_CENTRE_OFF_MAP 2u   /* the queried cell is not in the map */
#define FPE_MARGIN_NO_BAD         4u   /* dist_sq is FPE_MARGIN_NONE */
#define FPE_MARGIN_UNDER          8u   /* below mp.min_margin, by the expression above */
#define FPE_MARGIN_REFUSED        128u /* device forms: a cell the host forms refuse; every other field zero, FOOTHOLD not set */
typedef struct fpe_margin_params {    /* 24 bytes */
    int32_t classes;       /* FPE_MARGIN_* class bits, 1..15 */
    int32_t reach_cells;   /* 1..FPE_MARGIN_MAX_CELLS */
    double  min_margin;    /* metres; finite, >= 0; 0: no limit */
    int32_t reserved[2];   /* 0 */
} fpe_margin_params;
typedef struct fpe_margin_map_out {   /* 16 bytes; either may be NULL, not both */
    uint16_t* dist_sq;     /* [n_rows * n_cols] */
    int8_t*   nearest;     /* [n_rows * n_cols * 2] di, dj */
} fpe_margin_map_out;
typedef struct fpe_margin_query {     /* 8 bytes */
    int32_t row, col;
} fpe_margin_query;
typedef struct fpe_margin_record {    /* 8 bytes */
    uint16_t dist_sq;
    int8_t   di, dj;
    uint8_t  flags;         /* FPE_MARGIN_FOOTHOLD .. FPE_MARGIN_REFUSED */
    uint8_t  foot_id;       /* plan-bound: leg; open-loop: 0 */
    uint8_t  gait_cycle_id; /* plan-bound: g; open-loop: 0 */
    uint8_t  pad;
} fpe_margin_record;
typedef struct fpe_margin_summary {   /* 16 bytes; element b belongs to pose b */
    uint16_t min_dist_sq;
    uint8_t  min_cycle, min_leg;
    uint16_t n_footholds, n_under, n_off_map;
    uint8_t  first_under_cycle;  /* 255: none */
    uint8_t  pad[5];
} fpe_margin_summary;
typedef struct fpe_margin_out {       /* 16 bytes; either pointer may be NULL, not both */
    fpe_margin_record*  records;  /* [B * n_cycles * 4] */
    fpe_margin_summary* summary;  /* [B] */
} fpe_margin_out;
int fpe_margin_params_defaults(fpe_margin_params* out);
/* Dense: every cell of the region (roi NULL: the whole map).  Host arrays, synchronous / device arrays, asynchronous on `stream`. */
int fpe_margin_map(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const int32_t roi[4], const fpe_margin_map_out* out);
int fpe_margin_map_device(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const int32_t roi[4],
                          const fpe_margin_map_out* d_out, void* stream);
/* Open-loop: n arbitrary cells. */
int fpe_margin_cells(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const fpe_margin_query* queries, int32_t n,
                     fpe_margin_record* out);
int fpe_margin_cells_device(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const fpe_margin_query* d_queries,
                            int32_t n, fpe_margin_record* d_out, void* stream);
/* Plan-bound, device arrays: reads d_products->nominal (required) as a plan call on `stream` left it; `d_products` and `d_out`
 * themselves are host structs of device pointers.  Asynchronous on `stream`, behind whatever filled the product there. */
int fpe_margin_plan_device(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const fpe_plan_out* d_products, int32_t B,
                           int32_t n_cycles, const fpe_margin_out* d_out, void* stream);
/* Plan and check in one call, host arrays, synchronous: plans exactly as fpe_plan (strides NULL) or fpe_plan_strides would, checks the
 * plan on the same stream with no host synchronisation in between, on ONE snapshot, and returns the requested products (NULL: none)
 * and the margin outputs. */
int fpe_margin_plan(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const fpe_pose* poses, const fpe_stride* strides,
                    int32_t B, int32_t n_cycles, const fpe_plan_out* products, const fpe_margin_out* out);

/* ---- checked ranking: the swing, trunk and margin checks folded into the pick --------------------------------------------------------
 * BUILD-DEFINED.  fpe_plan_rank* scores a pose on commit counts, source counts, deviation and speed spread alone; a pose whose plan puts
 * the belly on a kerb ranks as well as a clean one.  One call plans the batch as fpe_plan_rank_strides does, reduces every pose's plan
 * to the three check summaries on the device — no check record is written or allocated anywhere on this path — folds them into the
 * ranking's class and score and returns the best K exactly as fpe_plan_rank does.
 * Parameters.  `checks` is a subset of FPE_CHECK_SWING | FPE_CHECK_TRUNK | FPE_CHECK_MARGIN (0 is allowed: no check runs); `reject` a
 * subset of checks | (checks ? FPE_CHECK_UNKNOWN : 0); the five weights are finite; `reserved` is +0.0 by its bits.  The blocks
 * `swing`, `trunk` and `margin` are the limits of fpe_swing_* / fpe_trunk_* / fpe_margin_*; the block of a disabled check is not read:
 * garbage there is not an error.  fpe_check_params_defaults: checks = all three, reject = 0, w_swing_over 10, w_lift 0, w_trunk_bad 10,
 * w_margin_under 1, w_unknown 1, the three blocks their own *_defaults — with which no OVER / UNDER / bad bit is ever set, so only the
 * unknown term acts until the caller sets limits.
 * Summaries.  With the products of the plan, S[b], T[b] and M[b] are, bit for bit, what fpe_swing_plan_device (start feet from
 * d_start_feet, else the `stance` product), fpe_trunk_plan_device and fpe_margin_plan_device write into summary[b] for the same
 * products, the same limit blocks and the snapshot current at entry.  REFUSED records are covered by this: those forms' rules hold.
 * Per pose:   unknown = (SWING ? S.n_unknown : 0) + (TRUNK ? T.n_unknown : 0) + (MARGIN ? M.n_off_map : 0), an int;
 *             hit = SWING iff enabled and S.n_over > 0 | TRUNK iff enabled and T.n_bad > 0 | MARGIN iff enabled and M.n_under > 0 |
 *                   UNKNOWN iff unknown > 0.
 * Score.  `base` is the f64 fpe_plan_rank / fpe_plan_rank_strides stores in score[b] for this pose (-0.0 already +0.0).  In f64, each
 * product first, added left to right, without contraction:
 *     v = base
 *     if SWING:   v = v + w_swing_over   * double(S.n_over);   v = v + w_lift * S.max_lift
 *     if TRUNK:   v = v + w_trunk_bad    * double(T.n_bad)
 *     if MARGIN:  v = v + w_margin_under * double(M.n_under)
 *     if checks:  v = v + w_unknown      * double(unknown)
 *     score = (v == 0.0) ? +0.0 : v
 * S.max_lift is always finite (0 without a segment).  T.min_clearance can be +infinity, and the pose-level M.min_dist_sq takes two or
 * three values on rough ground: there is no clearance and no distance term.
 * Class and order.  Class 2: the score is not finite.  Class 1: otherwise, gait_cycles_succeed < min_cycles or (hit & reject) != 0.
 * Class 0: the rest.  The order (class, score, pose index), the tie rule, the K bound, n_class0 and the gather are fpe_plan_rank's.
 * With checks == 0 every output of fpe_rank_out is byte-identical to fpe_plan_rank_strides with the same arguments.
 * Outputs.  fpe_rank_out as it is: `score` holds the checked score, `summary` the unchanged fpe_pose_summary.  Beside it fpe_check_out
 * (any pointer may be NULL): the three summaries (the array of a disabled check is left untouched), base_score and hit.
 * Records of the winners need no new call: best_products holds nominal, cycle_ok and stance of the K winners in K slots, and
 * fpe_swing_plan_device / fpe_trunk_plan_device / fpe_margin_plan_device take them with B = K.
 * Refusals (a refused call writes and queues nothing).  Everything fpe_plan_rank_strides[_device] refuses; for each ENABLED check
 * everything its *_plan_device form refuses at call level (a NaN limit, a bad radius, half extent or ride height, the box over the cell
 * cap, the unsupported map, the undecidable min_margin -> FPE_E_UNSUPPORTED, classes or reach out of range, reserved words), decided by
 * the same host functions; and, FPE_E_INVALID_ARG: bits outside the sets above, a non-finite weight, `reserved` not +0.0.
 * fpe_check_plan_device is the check stage alone, on products a plan call left on `stream`: nominal is required, cycle_ok with SWING or
 * TRUNK, and with SWING d_start_feet or the stance product.  It computes no score: it refuses (FPE_E_INVALID_ARG) a non-NULL
 * base_score, checks == 0, and a d_out without `hit` and without the summary array of any enabled check.
 * Conventions as fpe_plan_rank*: `rank` NULL and `checks` NULL mean the respective defaults; the host form is synchronous; the device
 * forms are asynchronous on `stream` and see the snapshot current at entry (the margin's bit planes are built on first use, on that
 * stream).  No atomics anywhere: every byte is a function of the inputs alone.
 * The checks in fpe_plan_beam*'s pruning: the checked beam below (fpe_plan_beam_checked*), which carries the partial-plan check state
 * from segment to segment.  Out of scope: fpe_multi_*, the service calls, the opt and centroid tracks. */
#define FPE_CHECK_SWING   1u
#define FPE_CHECK_TRUNK   2u
#define FPE_CHECK_MARGIN  4u
#define FPE_CHECK_UNKNOWN 8u
typedef struct fpe_check_params {     /* 160 bytes */
    uint32_t checks;       /* subset of SWING | TRUNK | MARGIN; 0 is allowed */
    uint32_t reject;       /* subset of checks | (checks ? FPE_CHECK_UNKNOWN : 0) */
    double   w_swing_over, w_lift, w_trunk_bad, w_margin_under, w_unknown;   /* all finite */
    double   reserved;     /* +0.0 (bits) */
    fpe_swing_limits  swing;    /* read only when SWING is enabled */
    fpe_trunk_limits  trunk;    /* read only when TRUNK is enabled */
    fpe_margin_params margin;   /* read only when MARGIN is enabled */
} fpe_check_params;
typedef struct fpe_check_out {        /* 40 bytes; any pointer may be NULL */
    fpe_swing_summary*  swing;       /* [B]; untouched when SWING is disabled */
    fpe_trunk_summary*  trunk;       /* [B]; untouched when TRUNK is disabled */
    fpe_margin_summary* margin;      /* [B]; untouched when MARGIN is disabled */
    double*             base_score;  /* [B]: the score before the check terms */
    uint8_t*            hit;         /* [B]: FPE_CHECK_* bits */
} fpe_check_out;
int fpe_check_params_defaults(fpe_check_params* out);
/* The check stage alone, device arrays: the three summaries and `hit`, no record array anywhere.  `d_products` and `d_out` themselves
 * are host structs of device pointers.  Asynchronous on `stream`, behind whatever filled the products there. */
int fpe_check_plan_device(fpe_handle h, const fpe_params* params, const fpe_check_params* checks, const fpe_plan_out* d_products,
                          const double* d_start_feet, int32_t B, int32_t n_cycles, const fpe_check_out* d_out, void* stream);
/* Plan, check and rank, device arrays; arguments as fpe_plan_rank_strides_device (d_strides and d_full may be NULL), d_check_out may be
 * NULL.  The start feet are the plan's stance. */
int fpe_plan_rank_checked_device(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_check_params* checks,
                                 const fpe_pose* d_poses, const fpe_stride* d_strides, int32_t B, int32_t n_cycles, int32_t K,
                                 const fpe_plan_out* d_full, const fpe_rank_out* d_out, const fpe_check_out* d_check_out, void* stream);
/* The same with host arrays, synchronous; arguments as fpe_plan_rank_strides (strides may be NULL), check_out may be NULL. */
int fpe_plan_rank_checked(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_check_params* checks,
                          const fpe_pose* poses, const fpe_stride* strides, int32_t B, int32_t n_cycles, int32_t K,
                          const fpe_rank_out* out, const fpe_check_out* check_out);

/* ---- checked beam: the swing, trunk and margin checks folded into the beam's pruning ------------------------------------------------
 * BUILD-DEFINED.  fpe_plan_beam* prunes on commit counts, sources, deviation and progress alone: it can drop the only stride sequence
 * that keeps the belly off a kerb.  Here every candidate carries the check state of its whole path — the three summaries over all
 * cycles of its ancestry — and that state enters the candidate's score and class in every segment.  No check record is written or
 * allocated anywhere, and nothing synchronises the host between segments.
 * Everything fpe_plan_beam defines stays: candidates, c = p * M + m, the segment penalty q, progress, n_s, the outputs, replay, dead
 * slots not written, no atomics.  `checks` is a fpe_check_params block with the checked ranking's rules.  On top of the beam:
 *  - Start feet of a root.  start_feet[b] (x, y, z of RF, RH, LH, LF) when given.  Otherwise, with state_in == NULL, the `stance`
 *    product of the root's plan (the same for every option; what fpe_plan_rank_checked uses).  With state_in != NULL and start_feet ==
 *    NULL the state carries no z: with SWING enabled the call is refused (FPE_E_INVALID_ARG); without SWING the start feet are +0.0
 *    (they only show in `feet`, for a leg whose path commits nothing).
 *  - Carried feet of a candidate.  Per leg, (x, y, double(z)) of the leg's `nominal` record of the latest cycle along the candidate's
 *    ancestry, this segment included, with cycle_ok != 0; when there is none, the root's start feet.  This is the plan-bound swing's
 *    rule for A applied across segment boundaries: a candidate whose segment commits nothing inherits its parent's feet.
 *    check_out.feet is this block of the final slots; a following call takes it as start_feet, together with out.state as state_in.
 *  - Path summaries of a candidate.  S_c, T_c, M_c: the three summaries over all (s + 1) * k cycles of the ancestry so far, the swing
 *    from the root's start feet.  Cycle indices g count from the BEAM's first cycle — first_over_cycle, first_bad_cycle,
 *    first_under_cycle and min_cycle; they are not state.cycle + g.
 *    THE CONTRACT.  For every live final slot, the summaries and `hit` in check_out are byte for byte what fpe_check_plan_device writes
 *    for the slot's products: nominal and cycle_ok of out.products, S * k cycles, the root's start feet, the same fpe_check_params,
 *    the same snapshot.  Everything that form inherits is covered by this: REFUSED records count as there; the margin reads
 *    nominal.valid and not cycle_ok, so valid feet of a failed cycle count; the "0 / +infinity / 65535 / 255 when there is none"
 *    rules apply.
 *  - unknown and hit: as in the checked ranking, from the path summaries.
 *  - Score.  P_c = P_parent + q stays the unchecked accumulation, output in base_penalty; it is the only thing a child inherits as
 *    P_parent: the check terms are never accumulated twice.  Then, in f64, each product first, added left to right, no contraction:
 *        v = P_c
 *        if SWING:   v = v + w_swing_over   * double(S_c.n_over);   v = v + w_lift * S_c.max_lift
 *        if TRUNK:   v = v + w_trunk_bad    * double(T_c.n_bad)
 *        if MARGIN:  v = v + w_margin_under * double(M_c.n_under)
 *        if checks:  v = v + w_unknown      * double(unknown)
 *        t = w_progress * cx;   score = v - t;   -0.0 is stored as +0.0
 *    out.penalty holds v.
 *  - Class and order.  Class 2: the score is not finite, ordered by c alone.  Class 1: otherwise, (hit & reject) != 0.  Class 0: the
 *    rest.  The order is (class, score, c) ascending.  n_s is unchanged, so a root whose candidates are all class 1 still fills its
 *    slots, by score.  Counts only grow along a path: a rejected candidate's descendants are rejected.
 *  - No checks.  With checks->checks == 0 every byte of fpe_beam_out equals fpe_plan_beam's, and check_out is not touched.
 *  - Refusals (nothing written or queued): everything fpe_plan_beam[_device] refuses; for each ENABLED check everything
 *    fpe_check_plan_device refuses at call level, decided by the same host functions (the unsupported map and the undecidable
 *    min_margin -> FPE_E_UNSUPPORTED included); the fpe_check_params bit, weight and `reserved` rules of the checked ranking; the
 *    missing start feet, above; and, the host form only, with SWING enabled: a start foot coordinate that is not finite or beyond
 *    +-1e6.  The device form cannot look at values: a bad start foot takes the swing record's own REFUSED path.
 * Conventions, snapshot semantics and asynchrony are those of fpe_plan_beam*: `beam` NULL and `checks` NULL mean the respective
 * defaults, check_out may be NULL; the margin's bit planes are acquired once, on the call's snapshot (built on first use, on the
 * call's stream).
 * Out of scope: a concatenation contract for checked beams, a global beam, fpe_multi_*, the service calls, the opt and centroid tracks. */
typedef struct fpe_beam_check_out {   /* 48 bytes; every pointer may be NULL; element b * W + w belongs to slot (b, w); dead slots are not written */
    fpe_swing_summary*  swing;        /* [B * W]; untouched when SWING is disabled */
    fpe_trunk_summary*  trunk;        /* [B * W]; untouched when TRUNK is disabled */
    fpe_margin_summary* margin;       /* [B * W]; untouched when MARGIN is disabled */
    double*             base_penalty; /* [B * W]: the accumulated penalty without the check terms */
    uint8_t*            hit;          /* [B * W]: FPE_CHECK_* bits */
    double*             feet;         /* [B * W * 4 * 3]: where the feet stand behind the last cycle, x, y, z of RF, RH, LH, LF */
} fpe_beam_check_out;
/* Host arrays; synchronous.  Arguments as fpe_plan_beam; start_feet: [B * 4 * 3] or NULL. */
int fpe_plan_beam_checked(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, const fpe_check_params* checks,
                          const fpe_pose* poses, const fpe_plan_state* state_in, const double* start_feet, int32_t B,
                          const fpe_stride* options, int32_t M, const fpe_beam_out* out, const fpe_beam_check_out* check_out);
/* Device arrays (every non-NULL pointer of d_out and d_check_out too); asynchronous on `stream`, as fpe_plan_beam_device. */
int fpe_plan_beam_checked_device(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, const fpe_check_params* checks,
                                 const fpe_pose* d_poses, const fpe_plan_state* d_state_in, const double* d_start_feet, int32_t B,
                                 const fpe_stride* d_options, int32_t M, const fpe_beam_out* d_out,
                                 const fpe_beam_check_out* d_check_out, void* stream);

/* ---- scan fusion: point clouds into the elevation layer on the device ---------------------------------------------------------------
 * BUILD-DEFINED (the reference's bring-up starts elevation_mapping ahead of the producer above, launch/mapping.launch:9-13; that
 * package is not part of the reference and no version is pinned: parity is against the build's own numpy statement,
 * tests/scan_reference.py).  One depth or lidar scan is fused into a robot-centric height map that lives in HBM, and the rectangle it
 * touched goes into the planner's snapshot through fpe_update_elevation_device without crossing the host link.  Every per-cell
 * reduction is an INTEGER reduction, so the result does not depend on the order in which the points arrive.
 *
 * 1. The scan state (fpe_scan_handle; owned by the engine it was created on; destroy it before that engine).  Two canonical device
 *    layers of one geometry {rows, cols, resolution, position}: `elevation` and `variance`, row-major, start index (0, 0).
 *    INVARIANT: in both layers a cell is unknown iff it holds the quiet NaN 0x7FC00000 (both layers hold it then).
 *     - create: every cell unknown.  Of `geom`, start_index must be (0, 0) and storage_order 1 (FPE_E_INVALID_ARG otherwise).
 *       Scratch of 16 bytes per state cell and a second pair of layer buffers are allocated here.
 *     - set_layers: rows * cols floats each, canonical; a cell that is NaN in either source becomes unknown in both layers.
 *     - read_layers: either pointer may be NULL, not both.
 *     - move: new cell (i, j) takes old cell (i + sr, j + sc) of both layers bit for bit, or becomes unknown where that lies outside
 *       (fpe_update_map's steps 1-2); |shift| >= size is valid; the geometry's position becomes `position` (finite).  The state
 *       holds a second buffer pair and swaps: nothing is shifted in place.
 *    Ordering: a state keeps an event behind its last operation and every operation waits GPU-side for it before its first kernel
 *    or copy, on whatever stream it runs (the filter scratch's pattern); the device forms never synchronise the host.  The host
 *    forms run on a stream of the state's and return complete.  Operations of one state serialise on the host.
 *
 * 2. Fusing one scan (fpe_scan_fuse[_device]).  THE CONTRACT.  Every product and every sum is rounded on its own (no contraction), in
 *    the order written; f32 divisions are IEEE.  T = scan->sensor_to_map, (xs, ys, zs) the point's three floats as doubles.
 *    Per point, in f64; the FIRST failing test decides the drop counter:
 *      1. dropped_nonfinite  if any of the three floats is not finite;
 *      2. dropped_range      unless  double(min_range) * double(min_range) <= (xs*xs + ys*ys) + zs*zs <= double(max_range) * double(max_range);
 *      3. xm = ((T0*xs + T1*ys) + T2*zs) + T3;  ym = ((T4*xs + T5*ys) + T6*zs) + T7;  zm = ((T8*xs + T9*ys) + T10*zs) + T11;
 *      4. dropped_height     unless  double(min_z) <= zm <= double(max_z);
 *      5. dropped_off_roi    unless  checkIfPositionWithinMap holds on both axes (t = -((x - position) - 0.5 * length); 0 <= t < length)
 *                            and the cell (getIndexFromPosition, -(int)(((x - 0.5 * length) - position) / resolution), the true
 *                            division) lies inside scan->roi;
 *      6. otherwise ACCEPTED, with q = (int32) rint(zm * 65536.0)   (|zm| <= 16384, so |q| <= 2^30).
 *    Per roi cell with accepted points:
 *      top = max q;  band_q = rint(double(band) * 65536.0), taken as 2^31 when it is larger (a band beyond 32768 m keeps every point);
 *      KEPT are the points with q >= top - band_q (in 64 bits): n their count, S the 64-bit sum of their q; the others count into
 *      below_band;  z_m = (float)((double(S) / double(n)) * (1.0 / 65536.0));
 *      dx = cx - T3, dy = cy - T7 with (cx, cy) the cell's centre (getPositionFromIndex: (position + (0.5 * length - 0.5 * resolution))
 *      + resolution * double(-index));  d2 = (float)(dx*dx + dy*dy), the sum in f64;
 *      v_m = max((var_base + var_range * d2) / (float)n, var_min)   in f32.
 *    Fusing with the prior (h, v) of the cell, in f32:
 *      prior unknown                       -> NEW:      h' = z_m;  v' = min(v_m, var_max)
 *      else d = z_m - h;  s = v + v_m;
 *        d*d > (gate*gate) * s             -> OUTLIER:  replace_count > 0 && n >= replace_count -> REPLACED: NEW's values;
 *                                                       otherwise h' = h;  v' = min(v + var_outlier, var_max)
 *        otherwise                         -> FUSED:    k = v / s;  h' = h + k*d;  v' = min(max(v - k*v, var_min), var_max)
 *    (min / max are fminf / fmaxf.  Should h' or v' come out NaN — a prior of infinities —, the cell becomes unknown in both layers:
 *    the invariant holds whatever the layers were set to.)  A cell with no accepted point is NOT WRITTEN: its bytes stay.
 *    info counts what the names say: n_points = scan->n_points = the five point classes' sum; cells_touched = cells_new + cells_fused +
 *    cells_outlier; cells_outlier INCLUDES cells_replaced; bbox in the state's indices.
 *    Refusals (nothing written, nothing queued; FPE_E_INVALID_ARG): null arguments (the device form's d_info may be NULL), n_points
 *    outside 0..FPE_SCAN_MAX_POINTS, point_stride < 3, a reserved field that is not 0, a roi that is empty or reaches outside the
 *    state, a non-finite transform or parameter, min_range > max_range, min_z > max_z, |min_z| or |max_z| > 16384, a negative
 *    variance parameter (var_base, var_range, var_min, var_max, var_outlier), var_min > var_max, gate <= 0, band < 0.
 *    fpe_scan_validate is that same routine without an engine (of `geom`: rows, cols, resolution).
 *    Forms.  Host: host points, host info (may be NULL), synchronous.  Device: device points, device info (16 int32; may be NULL),
 *    asynchronous on `stream`, never synchronises the host — except that the 8-byte point records of the passes grow on demand: the
 *    FIRST call of a state with a larger n_points than any before allocates (hipMalloc / hipFree, which synchronise the device).
 *    Three launches: scan_top_kernel (classify, integer max per cell, one 8-byte record per point), scan_sum_kernel (count and 64-bit
 *    sum of the kept points, integer atomics only), scan_fuse_kernel (one lane per roi cell: the rule above, both layers, info, and
 *    the cell's scratch words reset, so no call starts with a memset).  No float atomics anywhere.  fpe_set_tuning "scan_merge":
 *    0 (DEFAULT) the engine's choice, 1 the plain form (one atomic per point), 2 the merged form (runs of equal cells across
 *    adjacent lanes of a wavefront are reduced in registers first: one atomic per run); the outputs do not depend on it.
 *
 * 3. Into the planner's snapshot.
 *     - fpe_scan_install: the state's content becomes the engine's current snapshot: fpe_traversability_device on the state's
 *       elevation with the state's geometry and d_layers == NULL, then fpe_upload_map_device of that traversability and the elevation.
 *       fp == NULL: the defaults.  Returns what those two return.
 *     - fpe_scan_ingest_device, in this order: fpe_scan_move when `shift` is not (0, 0) or `position` differs from the state's; the
 *       fuse; fpe_update_elevation_device with that shift and position and ONE patch: scan->roi, pointing into the state's elevation
 *       layer (row-major with a pitch: row_stride = cols).  The snapshot is byte for byte what those three public calls leave.
 *       Refused as a whole (nothing moved, written, queued or installed): everything the fuse refuses; a non-finite position;
 *       FPE_E_NO_MAP before any map exists; FPE_E_INVALID_ARG when the snapshot's rows, cols or resolution differ from the state's;
 *       what fpe_update_elevation_device refuses for these filter parameters (fp == NULL: the defaults).  update_info may be NULL.
 *     - fpe_scan_ingest: the same with host points and a host scan info; synchronous.
 *    PROMISED: after an install and any sequence of ingests, fpe_read_map_layers' elevation equals the state's elevation bit for bit. */
#define FPE_SCAN_MAX_POINTS (1 << 22)
typedef struct fpe_scan_state* fpe_scan_handle;
typedef struct fpe_scan_params {   /* 48 bytes */
    float min_range, max_range;    /* on |p|^2 in the sensor frame */
    float min_z, max_z;            /* map-frame height window; |.| <= 16384 */
    float band;                    /* m below a cell's top that still counts as the surface */
    float var_base, var_range;     /* one point's variance at a cell: var_base + var_range * d2 */
    float var_min, var_max;
    float gate;                    /* sigmas */
    float var_outlier;             /* added to a cell's variance by a gated-out scan */
    int32_t replace_count;         /* a gated-out cell with >= this many kept points is replaced; 0 = never */
} fpe_scan_params;
typedef struct fpe_scan {          /* 128 bytes */
    double sensor_to_map[12];      /* row-major 3 x 4: m = R p + t */
    int32_t n_points;              /* 0 .. FPE_SCAN_MAX_POINTS */
    int32_t point_stride;          /* floats per point, >= 3; x, y, z first */
    int32_t roi[4];                /* row0, col0, n_rows, n_cols in the state's indices; non-empty, inside */
    int32_t reserved[2];           /* 0 */
} fpe_scan;
typedef struct fpe_scan_info {     /* 64 bytes, sixteen int32 */
    int32_t n_points, dropped_nonfinite, dropped_range, dropped_height, dropped_off_roi, accepted, below_band,
            cells_touched, cells_new, cells_fused, cells_outlier, cells_replaced;
    int32_t bbox[4];               /* row_min, col_min, row_max, col_max of touched cells; {0,0,-1,-1} when none */
} fpe_scan_info;
/* min_range 0.1, max_range 10, min_z -100, max_z 100, band 0.05, var_base 1e-4, var_range 1e-4, var_min 1e-6, var_max 1.0, gate 3,
 * var_outlier 1e-3, replace_count 0 */
int fpe_scan_params_defaults(fpe_scan_params* out);
int fpe_scan_validate(const fpe_map_desc* geom, const fpe_scan_params* sp, const fpe_scan* scan);   /* host arithmetic only; no engine */
int fpe_scan_create(fpe_handle h, const fpe_map_desc* geom, fpe_scan_handle* out);
int fpe_scan_destroy(fpe_scan_handle s);
int fpe_scan_geometry(fpe_scan_handle s, fpe_map_desc* out);
int fpe_scan_set_layers(fpe_scan_handle s, const float* elevation, const float* variance);                           /* host; synchronous */
int fpe_scan_set_layers_device(fpe_scan_handle s, const float* d_elevation, const float* d_variance, void* stream);
int fpe_scan_read_layers(fpe_scan_handle s, float* elevation, float* variance);                                      /* host; synchronous */
int fpe_scan_read_layers_device(fpe_scan_handle s, float* d_elevation, float* d_variance, void* stream);
int fpe_scan_move(fpe_scan_handle s, const int32_t shift[2], const double position[2], void* stream);                /* asynchronous */
int fpe_scan_fuse(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan* scan, const float* points, fpe_scan_info* info);
int fpe_scan_fuse_device(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan* scan, const float* d_points,
                         fpe_scan_info* d_info, void* stream);
int fpe_scan_install(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, void* stream);
int fpe_scan_ingest(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan* scan,
                    const float* points, const int32_t shift[2], const double position[2], fpe_scan_info* scan_info,
                    fpe_elevation_update_info* update_info);
int fpe_scan_ingest_device(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan* scan,
                           const float* d_points, const int32_t shift[2], const double position[2], fpe_scan_info* d_scan_info,
                           fpe_elevation_update_info* update_info, void* stream);

/* 4. Visibility clearing (fpe_scan_clear[_device]): cells a new scan SEES THROUGH become unknown.  The fuse can only grow obstacles: a
 *    cell is rewritten only by points that land in it, and a prior above what the scan sees is gated out.  What has left (a person, a
 *    door leaf, something tall seen at a grazing angle) therefore stays in the state until rays of a later scan pass below its height.
 *    BUILD-DEFINED like the fuse; the numpy statement is tests/scan_clear_reference.py.  THE CONTRACT, with point 2's conventions (f64,
 *    every product and sum rounded on its own, no contraction, the grid arithmetic of checkIfPositionWithinMap and
 *    getIndexFromPosition).  T = scan->sensor_to_map; the sensor's origin in the map frame is (T3, T7, T11).
 *    Per point i:
 *      1. strided_out     if i % ray_stride != 0; the point is not read;
 *      2. dropped_points  if one of point 2's tests 1-4 fails (non-finite, range, transform, height window; sp's limits).  A point that
 *                         passes is a RAY, wherever its end lies;
 *      3. dx = xm - T3, dy = ym - T7, dz = zm - T11;  m = fmax(fabs(dx), fabs(dy));  step = double(sample_step) * resolution;
 *         Kd = ceil(m / step);
 *      4. rays_long       if Kd > double(max_samples) (compared in f64); the ray is not walked;
 *      5. otherwise K = (int)Kd and the ray's samples are k = start_samples .. K - end_samples - 1; rays_empty if there are none.
 *         `rays` counts every ray, the long and the empty ones included;
 *      6. sample k: t = double(k) / double(K);  x = T3 + t*dx, y = T7 + t*dy, z = T11 + t*dz.  It is INSIDE iff
 *         checkIfPositionWithinMap holds on both axes and its cell lies in scan->roi (samples_in_roi counts these); an inside sample
 *         VIOLATES its cell iff the cell's prior elevation h is not NaN and (z + double(margin)) < double(h);
 *      7. a ray counts against a cell ONCE, however many of its samples violate it (hit_pairs counts these pairs; the cell's hits + 1).
 *         x and y are monotone in k, so a ray's samples in one cell are one run of consecutive k.
 *    Per roi cell: hits >= 1 counts into cells_hit; hits >= min_hits CLEARS the cell: both layers take 0x7FC00000, it counts into
 *    cells_cleared and lies in bbox (state indices).  Every other cell's bytes stay.  The prior is read by the ray pass and written
 *    only by the cell pass, and the only per-cell reduction is an integer count: the result does not depend on the order of the
 *    points (ray_stride == 1; above 1 the stride selects by index).
 *    Refusals (FPE_E_INVALID_ARG; nothing written, nothing queued): everything the fuse refuses for sp and scan; a null cp; a
 *    non-finite sample_step or margin; a field outside the range its comment gives; reserved != 0.  fpe_scan_clear_validate is that
 *    same routine without an engine.
 *    Forms: as the fuse's (host: host points, host info or NULL, synchronous; device: device points, device info of 64 bytes or NULL,
 *    asynchronous on `stream`, never synchronises the host).  Ordering as in point 1.  Two launches: a ray pass (integer atomics into
 *    the hits word of the cells' scratch, which is the fuse's `count` word: 0 at rest) and scan_clear_cells_kernel (one lane per roi
 *    cell: clears, puts the hits back to 0, writes the info from the last workgroup).  The state's scratch is at rest afterwards.
 *    fpe_set_tuning "scan_clear_form": 0 (DEFAULT) the engine's choice, 1 one lane per ray, 2 a group of adjacent lanes per ray;
 *    "scan_clear_group": the lanes per ray of form 2: 0 (DEFAULT) the engine's choice, 16, 32 or 64.  The outputs depend on neither.
 *     - fpe_scan_ingest_clear[_device]: fpe_scan_ingest[_device] with the clear between the move and the fuse: move (when the shift or
 *       the position says so), CLEAR, fuse, fpe_update_elevation_device with the one roi patch.  A cell that is cleared and hit by the
 *       same scan comes out NEW.  The snapshot is byte for byte what those four public calls leave; point 3's promise keeps holding
 *       (cleared cells lie inside the roi, and the patch carries their NaN).  Refused as a whole under fpe_scan_ingest's conditions
 *       plus the clear's.  clear_info, scan_info and update_info may each be NULL.
 *    (These declarations carry `extern`: tests/test_cpu_scan.py counts the lines that start with `int fpe_scan_` as the fifteen
 *    entry points of points 1-3.) */
typedef struct fpe_scan_clear_params {   /* 32 bytes */
    float   sample_step;    /* in cells, along the ray's dominant ground axis; 0 < . <= 1 */
    float   margin;         /* m a ray must pass BELOW a cell's height to count against it; >= 0 */
    int32_t start_samples;  /* samples skipped at the sensor's end; >= 0 */
    int32_t end_samples;    /* samples skipped at the point's end (the hit itself and its neighbourhood); >= 0 */
    int32_t min_hits;       /* rays that must count against a cell to clear it; >= 1 */
    int32_t ray_stride;     /* point i casts a ray iff i % ray_stride == 0; >= 1 */
    int32_t max_samples;    /* rays with more samples than this are not walked; 1 .. 65536 */
    int32_t reserved;       /* 0 */
} fpe_scan_clear_params;
/* defaults: 0.5, 0.10, 2, 4, 2, 1, 4096, 0 */
typedef struct fpe_scan_clear_info {     /* 64 bytes */
    int32_t n_points, strided_out, dropped_points, rays, rays_long, rays_empty, cells_hit, cells_cleared;
    int32_t bbox[4];        /* of the cleared cells, state indices; {0,0,-1,-1} when none */
    int64_t samples_in_roi, hit_pairs;
} fpe_scan_clear_info;
extern int fpe_scan_clear_params_defaults(fpe_scan_clear_params* out);
extern int fpe_scan_clear_validate(const fpe_map_desc* geom, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                                   const fpe_scan* scan);                                                /* host arithmetic only; no engine */
extern int fpe_scan_clear(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan,
                          const float* points, fpe_scan_clear_info* info);
extern int fpe_scan_clear_device(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan,
                                 const float* d_points, fpe_scan_clear_info* d_info, void* stream);
extern int fpe_scan_ingest_clear(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp,
                                 const fpe_scan_clear_params* cp, const fpe_scan* scan, const float* points, const int32_t shift[2],
                                 const double position[2], fpe_scan_clear_info* clear_info, fpe_scan_info* scan_info,
                                 fpe_elevation_update_info* update_info);
extern int fpe_scan_ingest_clear_device(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp,
                                        const fpe_scan_clear_params* cp, const fpe_scan* scan, const float* d_points,
                                        const int32_t shift[2], const double position[2], fpe_scan_clear_info* d_clear_info,
                                        fpe_scan_info* d_scan_info, fpe_elevation_update_info* update_info, void* stream);

/* 5. Gap closing (fpe_scan_close[_device]): small holes of the state's elevation bridged FOR THE PLANNER.  A fused scan is full of
 *    them (cells between two lidar rings, between the pixels of a depth image at range, cells the clear has just removed), and the
 *    filter chain and every check read an unknown cell as "no data".  The close is a PURE FUNCTION of the state's elevation layer: it
 *    never writes the state (an invented height never becomes the prior of a later fuse), reads no variance and produces none.
 *    BUILD-DEFINED like the fuse; the numpy statement is tests/scan_close_reference.py.  THE CONTRACT: all arithmetic is f32, every
 *    operation rounded on its own, no contraction, IEEE division.  A cell is KNOWN iff it lies inside the map and its elevation is not
 *    NaN (infinities are known); off the map counts as unknown.  The axes are a0 = (0, +1), a1 = (+1, 0), a2 = (+1, +1),
 *    a3 = (+1, -1), as (row, column) steps.  For every cell c of the requested rectangle:
 *      1. c known: the output takes the cell's bits;
 *      2. otherwise, per axis a: s+ is the least s in 1..reach for which c + s a is known, s- the same for c - s a (each search ends
 *         at the first known cell or at the map's edge); the axis SPANS iff both exist and s+ + s- - 1 <= max_gap; h+ and h- are its
 *         two end heights;
 *      3. n = the number of spanning axes; lo and hi = the least and the greatest end height over the spanning axes only;
 *      4. n == 0: no_support;  0 < n < min_axes: rejected_axes;  not ((hi - lo) <= max_spread): rejected_spread (a NaN difference
 *         is rejected here);
 *      5. otherwise the spanning axis with the least s+ + s-, the lowest axis number among equals, gives
 *         v = h- + (h+ - h-) * (float(s-) / float(s+ + s-));  a NaN v is rejected_spread, any other v FILLS the cell;
 *      6. every cell that is neither known nor filled takes the quiet NaN 0x7FC00000.
 *    fpe_scan_close[_device] writes the closed elevation of `rect` = {row0, col0, n_rows, n_cols} rectangle-local: element (r, c) at
 *    out[r * out_row_stride + c], out_row_stride >= n_cols.  cls may be NULL; given, it takes one byte per cell with the same pitch:
 *    0 known, 1 filled, 2 no_support, 3 rejected_axes, 4 rejected_spread.  Nothing outside the rectangle's elements is written, and
 *    neither the state's layers nor its scratch.  info may be NULL; cells = known + unknown, unknown = filled + no_support +
 *    rejected_axes + rejected_spread.  A closed value depends on the state only within `reach` cells.
 *    Refusals (FPE_E_INVALID_ARG; nothing written, nothing queued): a null state, kp, rect or out; a field outside the range its
 *    comment gives; a NaN or negative max_spread; a reserved word that is not 0; out_row_stride < n_cols; a rectangle that is empty
 *    or reaches outside the state.  fpe_scan_close_validate is that routine without an engine (of `geom` rows, cols, resolution).
 *    Forms: host (host out / cls / info, synchronous) and device (device buffers, a device info of 64 bytes, asynchronous on
 *    `stream`, never synchronises the host).  Ordering as in point 1: an operation of the state.  One launch per rectangle, in one of
 *    two forms of identical output, fpe_set_tuning "scan_close_form": 0 (DEFAULT) the engine's choice, 1 direct (one lane per cell,
 *    the searches through global memory), 2 tiled (a workgroup stages a 16 x 64 tile and a halo of `reach` in LDS).
 *     - fpe_scan_install_closed: fpe_scan_install with the closed whole-map layer in place of the state's elevation: the snapshot's
 *       elevation is close(state), its traversability the filter chain's answer for that.
 *     - fpe_scan_ingest_closed[_device]: move (when the shift or the position says so), the clear when cp != NULL, the fuse, the close
 *       of up to three rectangles, then ONE fpe_update_elevation_device whose patches carry the closed rectangles: (1) scan->roi
 *       grown by `reach` on every side, clipped to the map; (2) if sr > 0 the rows [0, reach), if sr < 0 the last `reach` rows, all
 *       columns; (3) the same for sc on the columns.  Later patches may overlap earlier ones; their values agree.  close_info
 *       describes rectangle (1).  Refused as a whole under fpe_scan_ingest_clear's conditions (without the clear's when cp == NULL)
 *       plus the close's, before anything is queued.  Every info may be NULL.
 *       PROMISED: after fpe_scan_install_closed and any sequence of fpe_scan_ingest_closed* calls with the same kp, the elevation
 *       fpe_read_map_layers returns equals close(whole state) bit for bit (off the map and unknown are the same thing to the close,
 *       so entering cells change nothing, and only the side whose neighbours left the map loses support).  Mixing these with
 *       fpe_scan_install / fpe_scan_ingest / fpe_scan_ingest_clear or with another kp VOIDS that promise: those write the state's own
 *       elevation into the snapshot, and the carried cells keep what the last call put there. */
typedef struct fpe_scan_close_params {   /* 32 bytes */
    int32_t reach;          /* cells searched along each direction; 1 .. 8 */
    int32_t max_gap;        /* unknown cells an axis may bridge (s+ + s- - 1); 1 .. 2 * reach - 1 */
    int32_t min_axes;       /* spanning axes a filled cell needs; 1 .. 4 */
    float   max_spread;     /* m between the least and the greatest end height; >= 0, may be +infinity, not NaN */
    int32_t reserved[4];    /* 0 */
} fpe_scan_close_params;
/* defaults: 4, 5, 2, 0.08 */
typedef struct fpe_scan_close_info {     /* 64 bytes */
    int32_t cells, known, unknown, filled, no_support, rejected_axes, rejected_spread, reserved;
    int32_t bbox[4];        /* of the filled cells, state indices; {0,0,-1,-1} when none */
    int32_t reserved2[4];
} fpe_scan_close_info;
extern int fpe_scan_close_params_defaults(fpe_scan_close_params* out);
extern int fpe_scan_close_validate(const fpe_map_desc* geom, const fpe_scan_close_params* kp, const int32_t rect[4]);  /* host arithmetic only; no engine */
extern int fpe_scan_close(fpe_scan_handle s, const fpe_scan_close_params* kp, const int32_t rect[4], float* out, int64_t out_row_stride,
                          uint8_t* cls, fpe_scan_close_info* info);
extern int fpe_scan_close_device(fpe_scan_handle s, const fpe_scan_close_params* kp, const int32_t rect[4], float* d_out,
                                 int64_t out_row_stride, uint8_t* d_cls, fpe_scan_close_info* d_info, void* stream);
extern int fpe_scan_install_closed(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_close_params* kp,
                                   void* stream);
extern int fpe_scan_ingest_closed(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp,
                                  const fpe_scan_clear_params* cp, const fpe_scan_close_params* kp, const fpe_scan* scan,
                                  const float* points, const int32_t shift[2], const double position[2],
                                  fpe_scan_clear_info* clear_info, fpe_scan_info* scan_info, fpe_scan_close_info* close_info,
                                  fpe_elevation_update_info* update_info);
extern int fpe_scan_ingest_closed_device(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp,
                                         const fpe_scan_clear_params* cp, const fpe_scan_close_params* kp, const fpe_scan* scan,
                                         const float* d_points, const int32_t shift[2], const double position[2],
                                         fpe_scan_clear_info* d_clear_info, fpe_scan_info* d_scan_info,
                                         fpe_scan_close_info* d_close_info, fpe_elevation_update_info* update_info, void* stream);

/* 6. Scan images (the *_image entry points): a depth camera's or a spinning lidar's image fused and cleared WITHOUT a point cloud.
 *    BUILD-DEFINED like points 2 - 5; the numpy statement is tests/scan_image_reference.py.  THE EQUIVALENCE: every image form writes,
 *    byte for byte, what its point form writes when given the points P of the image — a tight array of n_sel points, scan->n_points
 *    = n_sel, a stride of 3: both layers of the state, every word of every info record, the planner's snapshot.  The points are never
 *    materialised: no kernel of the image forms writes an x, y, z triple to memory, and a state allocates nothing per point beyond
 *    the 8-byte records it already has.
 *    SELECTED PIXELS: rows v = ri * row_step for ri = 0 .. nr - 1, nr = ceil(height / row_step); columns u = ci * col_step for
 *    ci = 0 .. nc - 1, nc = ceil(width / col_step); n_sel = nr * nc; the point ordinal is i = ri * nc + ci (the clear's ray_stride
 *    selects on i, as in point 4).
 *    THE POINT OF A PIXEL: all arithmetic is f32, every operation rounded on its own, no contraction, IEEE division (no reciprocal is
 *    multiplied in).  raw is the element at v * row_pitch + u.  U16: invalid iff raw == 0, d = float(raw) * depth_scale.  F32: invalid
 *    unless raw is finite and > 0, d = raw * depth_scale.  An invalid pixel is the point (NaN, NaN, NaN), which the fuse's test 1
 *    counts under dropped_nonfinite (fpe_scan_info keeps its sixteen words); a d that overflows meets the same test.
 *      pinhole:    x = ((float(u) - cx) * d) / fx;   y = ((float(v) - cy) * d) / fy;   z = d
 *      spherical:  (ce, se) = row_dir[2v], row_dir[2v + 1];  (ca, sa) = col_dir[2u], col_dir[2u + 1];
 *                  w = d * ce;   x = w * ca;   y = w * sa;   z = d * se
 *    The tables are data: the caller takes the cosines, the contract has no trigonometry.  scan->sensor_to_map maps that frame to the
 *    map.  Non-finite table entries are not refused (a device form cannot see them): their points are dropped_nonfinite.
 *    REFUSALS (FPE_E_INVALID_ARG; nothing written, nothing queued, nothing installed): everything the point form refuses for sp, cp,
 *    kp, scan, shift and position; a null im or image; a model or a format outside its two values; a width or height outside
 *    1 .. 4096; row_pitch < width; a step below 1; a depth_scale that is not finite or not > 0; pinhole: fx or fy not finite or 0, cx
 *    or cy not finite; spherical: a null table; a reserved word that is not 0; n_sel > FPE_SCAN_MAX_POINTS; scan->n_points != n_sel.
 *    scan->point_stride must pass the old check (>= 3) and is otherwise not read.  fpe_scan_image_validate is that routine without
 *    an engine (cp may be NULL: the fuse's refusals alone).
 *    FORMS, ordering, asynchrony and grow-on-demand allocation are the point forms'.  Host forms take a host image and host tables
 *    and stage them at their own size (2 or 4 bytes per pixel, plus the two tables); device forms take a device image, and row_dir /
 *    col_dir are device addresses.  fpe_scan_image_points (host only) writes the n_sel x 3 floats of the rule: the CPU-checkable
 *    statement of it.
 *     - fpe_scan_ingest_image[_device] is ONE routine for the three ingests: cp == NULL and kp == NULL: fpe_scan_ingest; cp given,
 *       kp == NULL: fpe_scan_ingest_clear; kp given (cp given or NULL): fpe_scan_ingest_closed, with its PROMISED statement and its
 *       voiding rule.  The order of operations and the patches are the existing ones.
 *    Kernels (csrc/fpe_scan_image.hpp): the top pass has one form, the merged one, and sums its five class counts per workgroup in
 *    LDS; the ray pass keeps both forms and "scan_clear_form" / "scan_clear_group" their meaning; "scan_merge" does not apply. */
#define FPE_SCAN_IMAGE_PINHOLE   0   /* optical frame: x right, y down, z forward */
#define FPE_SCAN_IMAGE_SPHERICAL 1   /* separable direction tables: a spinning lidar's range image */
#define FPE_SCAN_DEPTH_U16 0         /* uint16; 0 = no return */
#define FPE_SCAN_DEPTH_F32 1         /* float; valid iff finite and > 0 */
typedef struct fpe_scan_image {       /* 72 bytes */
    int32_t model, format;
    int32_t width, height;        /* pixels; 1 .. 4096 each */
    int32_t row_pitch;            /* ELEMENTS between rows; >= width (a crop is a pointer offset plus this) */
    int32_t row_step, col_step;   /* every row_step-th row and col_step-th column is a point; >= 1 */
    float   depth_scale;          /* metres per unit; finite, > 0 */
    float   fx, fy, cx, cy;       /* pinhole; fx, fy finite and not 0; cx, cy finite */
    int32_t reserved[2];          /* 0 */
    const float* row_dir;         /* spherical: height x {cos e, sin e}; host pointer in host forms, device pointer in device forms */
    const float* col_dir;         /* spherical: width  x {cos a, sin a} */
} fpe_scan_image;
extern int fpe_scan_image_validate(const fpe_map_desc* geom, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                                   const fpe_scan* scan, const fpe_scan_image* im);                 /* host arithmetic only; no engine */
extern int fpe_scan_image_points(const fpe_scan_image* im, const void* image, float* out_xyz);     /* host only */
extern int fpe_scan_fuse_image(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan* scan, const fpe_scan_image* im,
                               const void* image, fpe_scan_info* info);
extern int fpe_scan_fuse_image_device(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan* scan, const fpe_scan_image* im,
                                      const void* d_image, fpe_scan_info* d_info, void* stream);
extern int fpe_scan_clear_image(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan,
                                const fpe_scan_image* im, const void* image, fpe_scan_clear_info* info);
extern int fpe_scan_clear_image_device(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                                       const fpe_scan* scan, const fpe_scan_image* im, const void* d_image,
                                       fpe_scan_clear_info* d_info, void* stream);
extern int fpe_scan_ingest_image(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp,
                                 const fpe_scan_clear_params* cp, const fpe_scan_close_params* kp, const fpe_scan* scan,
                                 const fpe_scan_image* im, const void* image, const int32_t shift[2], const double position[2],
                                 fpe_scan_clear_info* clear_info, fpe_scan_info* scan_info, fpe_scan_close_info* close_info,
                                 fpe_elevation_update_info* update_info);
extern int fpe_scan_ingest_image_device(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp,
                                        const fpe_scan_clear_params* cp, const fpe_scan_close_params* kp, const fpe_scan* scan,
                                        const fpe_scan_image* im, const void* d_image, const int32_t shift[2],
                                        const double position[2], fpe_scan_clear_info* d_clear_info, fpe_scan_info* d_scan_info,
                                        fpe_scan_close_info* d_close_info, fpe_elevation_update_info* update_info, void* stream);

/* ---- host-side helpers (no GPU needed) -------------------------------------------------------- */
/* SpiralIterator visiting order as index offsets (di,dj) for rings 0..n_rings (generateRing walk,
 * consumed from the back).  Writes min(count, max_cells) entries of (di, dj, ring); returns count. */
int fpe_spiral_offsets(int32_t n_rings, int32_t* out_di_dj_ring, int32_t max_cells);
/* Half-width (cells) of the LDS tile a (searchRadius, footRadius, resolution) triple needs. */
int fpe_tile_halfwidth(float search_radius, float foot_radius, double resolution);
/* Algorithmic bytes per foothold used for the roofline:
 * 4*W^2 + 8*n_foot + 16 with W = 2*(floor(R/res+0.5)+floor(rf/res))+1. */
double fpe_algorithmic_bytes_per_foothold(float search_radius, float foot_radius, double resolution);

#ifdef __cplusplus
}
#endif
#endif /* FPE_H */
