// fpe_launch.hpp — the boundary between the host side of the engine (fpe_engine.cpp) and the kernel translation unit
// (fpe_kernels.hip and the family headers it includes): the ONE declaration of every fpe:: function the engine calls and the
// kernel side defines, the argument structs of the newer kernel families, and the only place for default arguments.
// fpe_kernels.hip includes this ahead of its own definitions, so a definition that drifts from its declaration — a changed
// parameter list, a struct field added on one side — no longer compiles or links; it cannot run with two layouts.
// (DevMap, PlanConsts, BitMap, FilterConsts, OptConsts: fpe_device.hpp.)
#pragma once
#include "fpe_device.hpp"

namespace fpe {

// ---- chained plans (fpe_plan_launch.hpp) ---------------------------------------------------------------------
// The optional per-pose arrays of a chained plan, and the form of every plan kernel they select, decided once:
//   strides            one fpe_stride per pose (fpe_plan_strides*, fpe_plan_rank_strides*): the kernels' stride instantiations;
//   stateIn / stateOut one fpe_plan_state per pose (fpe_plan_resume*): with either one the resume instantiations, which take a
//                      null strides as the plan's own stride;
//   none               the kernels as they were.
enum class PlanForm { Plain, Stride, Resume };
struct PlanChain {
    const fpe_stride* strides = nullptr;
    const fpe_plan_state* stateIn = nullptr;
    fpe_plan_state* stateOut = nullptr;
    PlanForm form() const { return (stateIn || stateOut) ? PlanForm::Resume : strides ? PlanForm::Stride : PlanForm::Plain; }
};
// What a chained-plan call launches.  None: no kernel of this form for the forced plan_group (`group` says which).
enum class PlanFamily { None, Lane8, Seq, Chained, Sequential };  // bit window: 8 lanes per leg | one wavefront per pose; direct: chained | sequential legs
struct PlanKernel {
    PlanFamily family;
    PlanForm form;
    int nrl, kw, winSide;  // bit-window families: rows per lane, words per row, window rows = columns
    int group;             // G of the direct families (plan_group_size), poses per workgroup of Seq (1 or 16)
    bool mid;              // the 3x3-only variant (Lane8, Chained<8>)
    int prod;              // compiled product mask (product_shape; Seq: 0 or 1)
    unsigned grid, block;
    size_t ldsBytes;
    int recSlots, slotBytes;  // Seq: cycles of staged records per pose, bytes of a pose's LDS slot
};
PlanKernel select_plan_kernel(const PlanConsts& pc, const MapGeom& g, bool bits, int B, int productShape, PlanForm form);
void describe_plan_kernel(const PlanKernel& k, char* buf, size_t n);
// bm: the snapshot's bit planes (the bit-window kernels), or null: the direct kernels
hipError_t launch_plan(const DevMap& m, const BitMap* bm, const PlanConsts& pc, const SpiralLut& lut, const fpe_pose* d_poses, int B,
                       int nCycles, const fpe_plan_out& d_out, const PlanChain& chain, hipStream_t stream);

// ---- direct kernels (fpe_kernels.hip) ------------------------------------------------------------------------
hipError_t launch_search_legs(const DevMap& m, const PlanConsts& pc, const SpiralLut& lut, const fpe_leg_query* d_q,
                              int n, fpe_foothold* d_out, hipStream_t stream);
// open-loop centroid method
hipError_t launch_centroid_legs(const DevMap& m, const PlanConsts& pc, float defaultR, const fpe_centroid_query* d_q, int n,
                                fpe_centroid_foothold* d_out, hipStream_t stream);
hipError_t launch_canonicalise(const float* d_src, float* d_dst, int rows, int cols, int si, int sj, int srcRowMajor, hipStream_t stream,
                               uint32_t* d_planeWords = nullptr, float thrDefault = 0.0f, float thrCandidate = 0.0f);
// ---- incremental map update (fpe_mapupdate.hpp) ----------------------------------------------------------------
// The argument block of map_update_kernel: the base snapshot's canonical layers, the new snapshot's, the shift (clamped by the
// engine to |sr| <= rows, |sc| <= cols: the same content, and i + sr cannot overflow), the patches in the order they are applied
// (device pointers; element (r, c) at r * rowStride + c * colStride) and the plane buffers of the carried threshold pairs.
// Layers travel as 32-bit patterns.
constexpr int kUpdateMaxPairs = 4;  // the sets a snapshot keeps (acquire_mask)
struct MapUpdatePatch {
    int32_t row0, col0, nr, nc;
    const uint32_t* trav;  // null: an elevation-only patch (fpe_update_elevation*): the traversability keeps the carried / cleared value
    const uint32_t* elev;
    int64_t rowStride, colStride;
};
struct MapUpdatePair {
    uint4* words;  // bitmap_words(rows, cols) units, padding zeroed by launch_map_update
    float thrD, thrC;
};
struct MapUpdateArgs {
    const uint32_t* baseTrav;
    const uint32_t* baseElev;
    uint32_t* dstTrav;
    uint32_t* dstElev;
    int32_t rows, cols, sr, sc;
    int32_t nPatches, nPairs;
    int32_t strideW, nw;  // set by launch_map_update
    MapUpdatePair pair[kUpdateMaxPairs];
    MapUpdatePatch patch[FPE_UPDATE_MAX_PATCHES];
};
hipError_t launch_map_update(const MapUpdateArgs& a, hipStream_t stream);
hipError_t set_max_lds(size_t planBytes, size_t searchBytes);
size_t plan_lds_bytes(const PlanConsts& pc);
size_t search_lds_bytes(const PlanConsts& pc);

// ---- bit-window path (fpe_bits.hpp) --------------------------------------------------------------------------
size_t bitmap_words(int rows, int cols, int* strideW, int* nw);
hipError_t launch_build_bitmap(const float* d_trav, int rows, int cols, float thrDefault, float thrCandidate,
                               uint32_t* d_words, hipStream_t stream);
bool bits_supported(const PlanConsts& pc, const MapGeom& g);

// ---- producer filters (fpe_filters.hpp) ----------------------------------------------------------------------
// What the host's description of the chain (fpe_host.cpp: filter_route and what follows from it — no GPU call, compiled for the
// host by the CPU tests) and the kernels share: the table limits, the shape a disc takes on the lattice, the LDS-size formulas the
// kernels carve their arrays with, and the rectangle lists of the region launches.
constexpr int kFT = 16;        // tile edge of the disc stencils
constexpr int kFilterMaxH = 24;  // largest halo the tables are sized for (e.g. r 0.115 m at 0.5 cm)
constexpr int kStepMaxClasses = 14;
constexpr int kStepMaxEdge = 24;
constexpr int kMomentMaxH = 12;
// The fused kernel's tile: 32 rows x 16 columns (512 threads) for halos up to eight cells, 32 x 32 beyond.  Rows amortise: the
// row runs of the step window are one per (tile row with halo, interior column), the prefix scans one lane per tile row.
constexpr int kFusedRows = 32;
constexpr int kFusedSmallMaxH = 8;
constexpr size_t kFilterMaxLds = 150 * 1024;  // dynamic LDS a filter kernel is given at most
// (TR x TC: the workgroup's cells — kFT x kFT for the walking kernels; 16 x 16, 32 x 16 (rows x columns) or 32 x 32 for the
// row-moment and row-run kernels)
__host__ __device__ inline size_t disc_lds_bytes(int H, int TR = kFT, int TC = kFT) {
    const int WR = TR + 2 * H, WC = TC + 2 * H;
    return static_cast<size_t>(WR) * WC * 4 + static_cast<size_t>(WR + WC) * 8 + static_cast<size_t>(TR + TC) * (2 * H + 1) * 8 + 2 * (TR + TC) * 4 + 16;
}
__host__ __device__ inline size_t step_lds_bytes(int H, int nClasses, int TR = kFT, int TC = kFT) {
    const int WR = TR + 2 * H;
    return ((disc_lds_bytes(H, TR, TC) + 15) & ~static_cast<size_t>(15)) + static_cast<size_t>(nClasses) * WR * TC * 8 + 128;
}
__host__ __device__ inline size_t fused_moment_bytes(int H, int TR, int TC) {
    const int WR = TR + 2 * H, W1 = TC + 2 * H + 1;
    return ((disc_lds_bytes(H, TR, TC) + 15) & ~static_cast<size_t>(15)) + 2 * static_cast<size_t>(WR) * W1 * 16;
}
// ---- the disc as a lattice SHAPE -------------------------------------------------------------------------------------------
// On the uniform lattice the members of a cell's disc are the same offsets for every cell — row offset o holds the columns
// |dc| <= w(o) — except for the few offsets that lie ON the circle ((0, R), (R, 0), (3, 4) R / 5 ...), where
// CircleIterator::isInside's rounding decides cell by cell.  step_shape sorts the offsets on the host: squared distance
// against r^2 with a relative margin of 1e-7 (position differences are good to 1e-12).
struct StepShape {
    int8_t rowW[2 * kFilterMaxH + 1 + 3];  // per row offset o + H: its robust half-width, -1: no robust member
    int8_t edgeR[kStepMaxEdge], edgeC[kStepMaxEdge];  // offsets on the circle
    uint32_t storeMask;                // bit w: some row has half-width w — the run is stored at that width; its class = the number of set bits below w
    int32_t nEdge, nClasses, wMax;
    int32_t ok;                        // 0: the shape does not fit the step kernels' tables (the walking kernels run)
    int32_t rowsOk;                    // 0: not even the rows' half-widths are to be trusted (map too far from the origin)
    uint64_t edgeRows;                 // bit o + H: row offset o holds an offset on the circle (complete also when the edge list overflowed)
};
// reach: the largest |coordinate| of a cell of the map — a position difference carries ~2 ulp of that, which decides how wide
// the band of offsets is that the per-cell arithmetic must settle.
StepShape step_shape(double r, double res, int H, double reach);
int filter_halo(double r, double res);
bool filters_supported(const FilterConsts& fc, const MapGeom& g);
int filter_reach_cells(const FilterConsts& fc, double res);  // R of fpe_update_elevation* (include/fpe.h)

// THE decision of a chain with these parameters on this geometry, made once per call (filter_route) and handed to everything that
// plans or launches: the halos and shapes, and the instantiation of each of the chain's launches.
struct WindowForm {  // a step window's launch
    enum Kind : int32_t { kWalk = 0, kRuns = 1, kInFused = 2 };  // the walking kernel | filter_step_runs*_kernel<TR, TC, HS> | rides in the fused launch
    int32_t kind, TR, TC, HS;
    size_t ldsBytes;
};
struct FusedForm {  // filter_fused*_kernel<H, kFusedRows, TC, HS>; H == 0: the separate normals / roughness kernels
    int32_t H, TC, HS;
};
struct FilterRoute {
    StepShape sN, s1, s2;
    int hN, hR, h1, h2;
    int tF;          // tile COLUMNS of the fused kernel (its rows: 32), 0: the moment form does not apply (walking kernels)
    int stepFused;   // the second step window rides in the fused kernel
    size_t fusedBytes;
    WindowForm first, second;
    FusedForm fused;
    // What a chain with these parameters can do without the caller's layer buffer: 1 = the two-launch chain that stores
    // step_height and traversability only (the fused kernel covers normals, slope, roughness and the second step window),
    // 0 = the intermediate layers have to exist (some filter runs as a launch of its own).
    int travOnly;
    // 1: region launches exist for this chain — it is the traversability-only one and its first window is the row-run kernel, as
    // in the full chain (which falls back to the walking kernel otherwise)
    int regionOk;
};
FilterRoute filter_route(const FilterConsts& fc, const MapGeom& g);

// Region launches of the traversability-only chain (fpe_update_elevation*): the same two kernels' bodies over the tiles of the
// GLOBAL tile grid that a list of tile rectangles names, passed in the kernel arguments (no host-to-device copy).
constexpr int kRegionMaxRects = 12;  // 8 patches + 4 bands
struct TileRect {
    int32_t ty0, tx0, ny, nx;  // tiles [ty0, ty0 + ny) x [tx0, tx0 + nx) of the launch's tile grid
};
struct TileRects {
    int32_t n, nBlocks;  // rectangles used; workgroups of the launch = the sum of ny * nx
    TileRect r[kRegionMaxRects];
};
struct CellRect {
    int32_t r0, c0, r1, c1;  // cells [r0, r1) x [c0, c1)
};
struct FilterRegion {
    TileRects fused;      // tiles of the fused launch: every tile that intersects a dirty rectangle
    TileRects step;       // tiles of the step-height launch: those tiles' cells grown by the second step window's halo
    int64_t recomputed;   // cells of the fused launch's tiles (the union, clipped to the map): what the chain stores
};
// Host arithmetic only.  false: no region launches for this route (FilterRoute::regionOk) or more than kRegionMaxRects
// rectangles — the caller runs the full chain.
bool filters_region_plan(const MapGeom& g, const FilterRoute& rt, const CellRect* dirty, int nDirty, FilterRegion* out);
// Cells of the union of `n` rectangles (clipped to rows x cols)
int64_t cell_rects_union(const CellRect* r, int n, int rows, int cols);
// The chain on `stream`: step heights, then normals + slope + roughness + second step window + weighted sum in one launch
// (filter_fused_kernel); launches of their own for whatever the lattice forms do not cover.  travOnly: only L.stepHeight and
// L.trav are valid pointers (rt.travOnly must say yes).  region: null, or the tiles to run (rt.regionOk; travOnly) — the
// region kernels of the same forms.
hipError_t launch_filters(const MapGeom& g, const FilterConsts& fc, const FilterRoute& rt, const float* d_elev, const FilterLayers& L, bool travOnly,
                          const FilterRegion* region, hipStream_t stream);

// ---- opt track (fpe_opt.hpp) ---------------------------------------------------------------------------------
hipError_t launch_opt_track(const DevMap& m, const PlanConsts& pc, const OptConsts& oc, const fpe_pose* d_poses, int B, int nCycles,
                            const uint8_t* d_cycleOk, const fpe_opt_out& d_out, hipStream_t stream, uint32_t* doneFlag = nullptr, uint32_t doneValue = 0);

// ---- dense foothold map (fpe_footmap.hpp) --------------------------------------------------------------------
// Region of a foothold-map call in canonical indices (fpe_foothold_map's roi)
struct FootmapRoi {
    int row0, col0, nr, nc;
};
int foothold_map_supported(const PlanConsts& pc, const MapGeom& g);
hipError_t launch_foothold_map(const DevMap& m, const BitMap& bm, const PlanConsts& pc, const FootmapRoi& roi, uint8_t* d_flags,
                               float* d_height, hipStream_t stream);

// ---- dense snap map (fpe_footsnap.hpp) -----------------------------------------------------------------------
// Host-proved constants of a snap call (snap_prove in fpe_engine.cpp)
struct SnapConsts {
    int32_t nRings, nCand;  // SpiralIterator rings of R and rank-table entries of rings 0..nRings
    int32_t ringT;          // the outer two rings' isInside test: di^2 + dj^2 <= ringT
    int32_t rectA, rectB;   // rectangle: |di| <= rectA and |dj| <= rectB inside (cell-centre offsets)
    float Rf;               // the search radius
    int32_t polyKind;       // 0 rectangle, 1 hexagon (query construction of the literal path)
};
bool foothold_snap_bits_ok(const PlanConsts& pc, const SnapConsts& sc, bool haveBits, bool rectProved);
hipError_t launch_foothold_snap_bits(const DevMap& m, const BitMap& bm, const PlanConsts& pc, const SnapConsts& sc, const SpiralLut& lut,
                                     const FootmapRoi& roi, int8_t* d_offset, uint8_t* d_source, float* d_z, hipStream_t stream);
size_t foothold_snap_literal_scratch_bytes();
hipError_t launch_foothold_snap_literal(const DevMap& m, const PlanConsts& pc, const SnapConsts& sc, const SpiralLut& lut,
                                        const FootmapRoi& roi, void* scratch, int8_t* d_offset, uint8_t* d_source, float* d_z,
                                        hipStream_t stream);

// ---- dense centroid map (fpe_centroidmap.hpp) ----------------------------------------------------------------
// Host-derived constants of a dense centroid call (centroid_map_consts)
struct CmapConsts {
    float Rf;         // the search radius: the rectangle is {2 Rf, Rf} (cpp:1616-1617)
    int32_t H;        // reach of the rectangle from its cell, rows or columns: ceil(Rf / res) + 2
    int32_t rb, re;   // map rows [rb, re) of the planes: the region's rows +- H, clipped to the map
    int32_t nwr;      // words per plane column: ceil((re - rb) / 32)
};
bool centroid_map_consts(const MapGeom& g, const FootmapRoi& roi, float R, CmapConsts& cc);
size_t centroid_map_scratch_bytes(const FootmapRoi& roi, const CmapConsts& cc);
hipError_t launch_centroid_map(const DevMap& m, const PlanConsts& pc, const CmapConsts& cc, const FootmapRoi& roi, void* scratch,
                               uint8_t* d_code, int8_t* d_offset, float* d_z, hipStream_t stream);

// ---- the products of a plan call --------------------------------------------------------------------------------
// Described ONCE, for both sides: the eight of fpe_plan_out, then the four of fpe_opt_out, in field order — which is also the
// order of the arenas that FootholdPlanner.plan_outputs(pinned=True) relies on (its one pinned block then leaves in one transfer,
// copy_out).  The engine's sizes, offsets, device-side structs and copy segments (plan_host, the ranking's and the beam's layouts)
// and the kernel side's copy table (plan_copies, fpe_rank.hpp) all follow this table: a new product is a line here beside its
// field in include/fpe.h — and, where a ranking or a beam has to plan it for its own reading, a flag in that layout's reads[].
enum ProductScale { kPerLeg, kPerCycle, kPerPose };  // elements: pose x cycle x leg, pose x cycle, pose
struct Product {
    size_t elemBytes;
    ProductScale scale;
};
constexpr int kPlanProducts = 8, kOptProducts = 4, kProducts = kPlanProducts + kOptProducts;
constexpr Product kProductTable[kProducts] = {
    {sizeof(fpe_foothold), kPerLeg},            // fpe_plan_out: nominal
    {sizeof(fpe_centroid_foothold), kPerLeg},   //   centroid
    {3 * sizeof(double), kPerLeg},              //   default_next
    {1, kPerCycle},                             //   cycle_ok
    {12 * sizeof(double), kPerPose},            //   stance
    {sizeof(fpe_selected_foothold), kPerLeg},   //   selected
    {1, kPerPose},                              //   pose_status
    {sizeof(fpe_selected_packed), kPerLeg},     //   selected_packed
    {sizeof(fpe_opt_foothold), kPerLeg},        // fpe_opt_out: footholds
    {sizeof(fpe_opt_cycle), kPerCycle},         //   cycles
    {1, kPerPose},                              //   gate_fail_cycle
    {2 * sizeof(double), kPerPose},             //   rows_after
};
constexpr int kCycleOk = 3;  // the one product the engine itself reads (the opt track's input, the speculative call's check)
constexpr size_t product_bytes(int k, size_t B, size_t nCycles) {
    return kProductTable[k].elemBytes * B *
           (kProductTable[k].scale == kPerPose ? 1 : (kProductTable[k].scale == kPerCycle ? nCycles : nCycles * 4));
}
// The one place that views the two structs as arrays of pointers: slot k of fpe_plan_out = product k of the table, slot k of
// fpe_opt_out = product kPlanProducts + k.
static_assert(sizeof(fpe_plan_out) == kPlanProducts * sizeof(void*), "fpe_plan_out: one pointer per product of the table");
static_assert(sizeof(fpe_opt_out) == kOptProducts * sizeof(void*), "fpe_opt_out: one pointer per product of the table");
static_assert(offsetof(fpe_plan_out, cycle_ok) == kCycleOk * sizeof(void*), "kCycleOk names fpe_plan_out::cycle_ok");
inline void** slots(fpe_plan_out& o) { return reinterpret_cast<void**>(&o); }
inline void* const* slots(const fpe_plan_out& o) { return reinterpret_cast<void* const*>(&o); }
inline void** slots(fpe_opt_out& o) { return reinterpret_cast<void**>(&o); }
inline void* const* slots(const fpe_opt_out& o) { return reinterpret_cast<void* const*>(&o); }

// ---- ranking of a planned batch (fpe_rank.hpp) ---------------------------------------------------------------
struct RankConsts {
    double wFail, wSpiral, wNone, wDeviation, wSpeedSpread;
    double stepHalf;  // double(stepLength / 2): the current feet start at stance - stepHalf (setFirstGait, cpp:2679-2699)
    int32_t minCycles;
    int32_t rfFirst;
};
size_t rank_scratch_bytes(int B, int K);
struct CheckStage;  // (the checked ranking, below)
// d_strides: one fpe_stride per pose, the stride form of the call (fpe_plan_rank_strides*); null: the kernels as they were.
// check: the check stage of fpe_plan_rank_checked*, launched between the summary and the select on the summary's score, pose
// summary and keys; null: none.
hipError_t launch_rank(const RankConsts& rc, const fpe_pose* d_poses, int B, int nCycles, int K, const fpe_plan_out& full,
                       fpe_pose_summary* d_summary, double* d_score, void* scratch, int32_t* d_best, int32_t* d_nClass0,
                       const fpe_plan_out& bestProducts, hipStream_t stream, const fpe_stride* d_strides = nullptr,
                       const CheckStage* check = nullptr);
hipError_t set_max_lds_rank();

// ---- the dense maps as message layers (fpe_layers.hpp) -------------------------------------------------------
// What a layer reads: a canonical product of the region, element (r, c) at r * nc + c (times 2, plus the component, for the
// interleaved int8 offset pairs)
enum LayerSrcKind : int32_t { kLayerSrcU8 = 0, kLayerSrcI8Pair0 = 1, kLayerSrcI8Pair1 = 2, kLayerSrcF32 = 3 };
struct LayerSlot {
    const void* src;  // the canonical product (device)
    float* dst;       // rows * cols floats of the whole map (device)
    int32_t kind;     // LayerSrcKind
    int32_t pad;
};
// The argument block of layers_export_kernel: the whole map, the destination layout, the region, one slot per layer
struct LayersArgs {
    int32_t rows, cols;    // the whole map
    int32_t si, sj;        // start index of the destination buffers: 0 <= si < rows, 0 <= sj < cols
    int32_t dstRowMajor;   // 1 row-major, 0 column-major destinations
    int32_t nLayers;       // slots used
    int32_t vec16;         // set by launch_layers_export: the 16-byte store path holds for every destination
    int32_t pad;
    FootmapRoi roi;
    LayerSlot slot[FPE_LAYER_COUNT];
};
hipError_t launch_layers_export(const LayersArgs& a, hipStream_t stream);

// ---- beam search over stride options (fpe_beam.hpp) ----------------------------------------------------------
struct BeamConsts {
    double wFail, wSpiral, wNone, wDeviation, wProgress;
};
// B roots, M options, W entries kept per root, S segments of k cycles.  slotStride: slots per root of the survivor, parent and
// history arrays (the final beam's live entries, n_{S-1}: no segment keeps more); outStride: slots per root of the outputs (W in the
// caller's arrays; the host form's arena is dense, n_{S-1}).
struct BeamShape {
    int32_t B, M, W, S, k;
    int32_t slotStride, outStride;
};
// One kept candidate of a segment: where it came from, its accumulated penalty and its score
struct BeamSurvivor {
    int32_t parent, option;
    double penalty, score;
};
// The device scratch of a beam call (laid out by the engine).  chains: B * n_{S-2} * M, the most one segment plans.
struct BeamScratch {
    fpe_pose* poses;            // [chains] the candidates' poses, strides and states: what the segment's plan call reads ...
    fpe_stride* strides;
    fpe_plan_state* stateIn;
    fpe_plan_state* stateOut;   // ... and writes, with
    fpe_plan_out cand;          // its products: nominal, default_next and cycle_ok (scoring reads them) and every requested one
    double* candPenalty;        // [chains]
    double* candScore;          // [chains]
    void* keys;                 // [chains] 16-byte sort keys
    BeamSurvivor* surv;         // [S][B][slotStride]
    fpe_plan_state* parents;    // [B][slotStride] the states behind the last segment's survivors
    fpe_plan_out hist;          // [S][B][slotStride] blocks of k cycles: the requested products only
    void* candCheck;            // [chains] the candidates' check states, kBeamCheckStateBytes each (a checked beam only: fpe_beam_check.hpp)
    void* parentsCheck;         // [B][slotStride] those behind the last segment's survivors
};
int beam_live(const BeamShape& sh, int s);  // n_s = min(W, M^(s+1)): entries every root keeps behind segment s
// Segment s: the candidates' inputs from the survivors of segment s - 1 (s = 0: from d_stateIn, or — null — none: the chains start
// from the poses) ...
hipError_t launch_beam_expand(const BeamShape& sh, int s, const fpe_pose* d_poses, const fpe_stride* d_options,
                              const fpe_plan_state* d_stateIn, const BeamScratch& sc, hipStream_t stream);
// ... and, behind the segment's plan call, score, select and keep
hipError_t launch_beam_prune(const BeamConsts& bc, const BeamShape& sh, int s, const BeamScratch& sc, hipStream_t stream);
// Behind the last segment: every live slot's path, products, state, score and penalty, and n_live
hipError_t launch_beam_trace(const BeamShape& sh, const BeamScratch& sc, const fpe_beam_out& d_out, hipStream_t stream);

// ---- swing checks (fpe_swing.hpp) ----------------------------------------------------------------------------
// The limits of a call as the kernels take them, by value, checked by the host (no NaN): max_length already squared, and the radius
// of a segment that names none already resolved (limits.radius, else params.footRadius; finite, <= FPE_SWING_MAX_RADIUS).
struct SwingConsts {
    double maxLift, maxRise, maxLengthSq;
    float defaultRadius;
    int32_t pad;
};
bool swing_map_supported(const MapGeom& g);  // the maps the kernels' cell enumeration is proven on (fpe_swing.hpp)
hipError_t launch_swing_segments(const DevMap& m, const SwingConsts& sc, const fpe_swing_query* d_q, int n, fpe_swing_record* d_out,
                                 hipStream_t stream);
// The segments a plan's products imply: B * nCycles * 4 records (required) and, where d_summary is given, one summary per pose
hipError_t launch_swing_plan(const DevMap& m, const SwingConsts& sc, const fpe_foothold* d_nominal, const uint8_t* d_cycleOk,
                             const double* d_startFeet, int B, int nCycles, fpe_swing_record* d_records, fpe_swing_summary* d_summary,
                             hipStream_t stream);

// ---- trunk checks (fpe_trunk.hpp) ----------------------------------------------------------------------------
// The limits of a call as the kernels take them, by value, checked by the host (no NaN; rideHeight finite), and the box of a stance
// that names none already resolved (the limits' half extents, else half of params.length / params.width; finite, in
// (0, FPE_TRUNK_MAX_HALF_EXTENT]).
struct TrunkConsts {
    double minClearance, maxSlopeX, maxSlopeY, rideHeight;
    double defaultHx, defaultHy;
};
bool trunk_box_supported(double hx, double hy, double res);  // the cell cap of include/fpe.h (FPE_TRUNK_MAX_CELLS)
// Whether a host form refuses the stance: the expressions the kernel answers FPE_TRUNK_REFUSED by
bool trunk_stance_refused(const TrunkConsts& tc, const fpe_trunk_query& q, double res);
hipError_t launch_trunk_stances(const DevMap& m, const TrunkConsts& tc, const fpe_trunk_query* d_q, int n, fpe_trunk_record* d_out,
                                hipStream_t stream);
// The stances a plan's products imply: B * nCycles records (required) and, where d_summary is given, one summary per pose
hipError_t launch_trunk_plan(const DevMap& m, const TrunkConsts& tc, const fpe_foothold* d_nominal, const uint8_t* d_cycleOk, int B,
                             int nCycles, fpe_trunk_record* d_records, fpe_trunk_summary* d_summary, hipStream_t stream);

// ---- edge margin (fpe_margin.hpp) ----------------------------------------------------------------------------
// The parameters of a call as the kernels take them, by value, checked by the host: the class bits (1..15), the reach in cells
// (1..FPE_MARGIN_MAX_CELLS), and the two sides of the limit's comparison, each formed once in f64 (res2 = g.res * g.res,
// minMargin2 = min_margin * min_margin).
struct MarginConsts {
    int32_t classes, reach;
    double res2, minMargin2;
};
// Whether a host form refuses the cell: the expression the kernel answers FPE_MARGIN_REFUSED by
bool margin_query_refused(int rows, int cols, const fpe_margin_query& q);
int margin_lanes_log2(int reach);  // lanes per query of margin_cells_kernel, as a power of two
hipError_t launch_margin_map(const BitMap& bm, const MapGeom& g, const MarginConsts& mc, const FootmapRoi& roi, uint16_t* d_distSq,
                             int8_t* d_nearest, hipStream_t stream);
hipError_t launch_margin_cells(const BitMap& bm, const MapGeom& g, const MarginConsts& mc, const fpe_margin_query* d_q, int n,
                               fpe_margin_record* d_out, hipStream_t stream);
// The footholds a plan's nominal product holds: B * nCycles * 4 records (required) and, where d_summary is given, one summary per pose
hipError_t launch_margin_plan(const BitMap& bm, const MapGeom& g, const MarginConsts& mc, const fpe_foothold* d_nominal, int B, int nCycles,
                              fpe_margin_record* d_records, fpe_margin_summary* d_summary, hipStream_t stream);

// ---- checked ranking (fpe_check.hpp) -------------------------------------------------------------------------
// The argument block of plan_check_kernel: the enabled checks with their constants (those of a disabled check are not read), the
// weights, the products read and the outputs (null: not wanted).  The last four are the ranking's: launch_rank fills them in from
// its own arguments; launch_plan_check alone (fpe_check_plan_device) leaves them null.
struct CheckArgs {
    uint32_t checks, reject;  // FPE_CHECK_* bits
    double wSwingOver, wLift, wTrunkBad, wMarginUnder, wUnknown;
    SwingConsts sc;
    TrunkConsts tc;
    MarginConsts mc;
    int32_t marginLanesLog2;  // margin_lanes_log2(mc.reach)
    int32_t minCycles;        // the ranking's class-1 threshold
    const fpe_foothold* nominal;
    const uint8_t* cycleOk;
    const double* startFeet;  // B * 4 * 3: the caller's, else the stance product
    fpe_swing_summary* swing;
    fpe_trunk_summary* trunk;
    fpe_margin_summary* margin;
    double* baseScore;
    uint8_t* hit;
    const fpe_pose_summary* poseSummary;
    double* score;
    void* keys;  // RankKey[B] (fpe_rank.hpp)
};
// What a check stage launches with: the snapshot's layers, the margin's planes (not read without FPE_CHECK_MARGIN) and the block
struct CheckStage {
    DevMap m;
    BitMap bm;
    CheckArgs a;
};
// rank: the form behind rank_summary_kernel (reads score and poseSummary, writes score and keys), else the summaries and hit alone
hipError_t launch_plan_check(const CheckStage& st, int B, int nCycles, bool rank, hipStream_t stream);


// ---- checked beam (fpe_beam_check.hpp) -----------------------------------------------------------------------
constexpr size_t kBeamCheckStateBytes = 208;  // one candidate's or parent's check state (BeamCheckState)
// What beam_check_kernel takes beside the check stage's block.  The engine fills in bc, rootFeet and rootFeetStride;
// launch_beam_prune_checked the rest, from the shape, the segment and the scratch.
struct BeamCheckArgs {
    int32_t nPrev, M, k, slotStride, seg;
    int32_t rootFeetStride;      // doubles from one root's start feet to the next root's
    BeamConsts bc;
    const double* defaultNext;
    const fpe_plan_state* stateOut;
    const void* parents;         // the parents' check states; null in segment 0, which starts from
    const double* rootFeet;      // the roots' start feet: the caller's, else the stance the segment's plan wrote (null: none, +0.0)
    void* cand;
    double* candPenalty;
    double* candScore;
    void* keys;
};
// Segment s behind its plan call: check and score (waves: 1 or 4 wavefronts per candidate), select, keep — launch_beam_prune's
// three launches with the checks folded in
hipError_t launch_beam_prune_checked(const BeamShape& sh, int s, const BeamScratch& sc, const CheckStage& st, const BeamCheckArgs& args,
                                     int waves, hipStream_t stream);
// launch_beam_trace with the check outputs (d_checkOut: device pointers, null: not wanted) of the enabled `checks`
hipError_t launch_beam_trace_checked(const BeamShape& sh, const BeamScratch& sc, const fpe_beam_out& d_out, uint32_t checks,
                                     const fpe_beam_check_out& d_checkOut, hipStream_t stream);

// ---- scan fusion (fpe_scan.hpp) ------------------------------------------------------------------------------
// The scratch of one state cell between the passes of a fuse, indexed by the cell's LOCAL index in the call's roi (r * nc + c, which
// is below rows * cols): 16 bytes, at rest {kScanTopNone, 0, 0} — written so at create, and again by scan_fuse_kernel for every cell
// a call touched.
struct alignas(16) ScanCell {
    int32_t top;    // max q of the accepted points (atomicMax)
    uint32_t count;  // kept points
    int64_t sum;     // their q, summed
};
static_assert(sizeof(ScanCell) == 16, "16 bytes of scratch per state cell (include/fpe.h)");
constexpr int32_t kScanTopNone = INT32_MIN;
constexpr uint32_t kScanNoCell = 0xFFFFFFFFu;  // the record of a dropped point
// The accumulators of a call's info between its passes (device, 32 words, owned by the state): words 0-15 are fpe_scan_info's, at
// rest 0 but for the bbox minima (INT32_MAX) and maxima (-1); word 16 is scan_fuse_kernel's ticket (at rest 0).  The last workgroup of
// scan_fuse_kernel takes the totals out with atomic exchanges that put the rest values back, and writes the caller's info.
constexpr int kScanAccWords = 32;
constexpr int kScanTicket = 16;
// The point source of the image forms (fpe_scan_*_image*; fpe_scan_image.hpp), by value at the END of both argument blocks: the
// descriptor's fields with device addresses.  data == null: the call's points are `points` with `stride`.
struct ScanImage {
    const void* data;      // uint16 or float elements
    const float* rowDir;   // spherical: height x {cos e, sin e}
    const float* colDir;   // spherical: width x {cos a, sin a}
    int32_t model, format;
    int32_t pitch;         // elements between rows
    int32_t rowStep, colStep;
    int32_t selCols;       // selected columns: ceil(width / colStep); the point ordinal is ri * selCols + ci
    float scale, fx, fy, cx, cy;
};
// The argument block of the three passes, by value: the contract's constants formed once on the host (the squares and widenings of
// include/fpe.h), the state's geometry, the roi and the buffers.
struct ScanArgs {
    double T[12];
    double minR2, maxR2, minZ, maxZ;
    MapGeom g;
    int64_t bandQ;  // min(rint(double(band) * 65536), 2^31)
    float varBase, varRange, varMin, varMax, gate2, varOutlier;  // gate2 = gate * gate (f32)
    int32_t replaceCount;
    int32_t n, stride;
    int32_t row0, col0, nr, nc;
    const float* points;
    uint2* rec;       // [n]: (local cell or kScanNoCell, q)
    ScanCell* cells;  // [rows * cols]
    int32_t* acc;     // [kScanAccWords]
    uint32_t* elev;   // the state's layers, as 32-bit patterns
    uint32_t* var;
    int32_t* info;    // the caller's fpe_scan_info (device), or null
    ScanImage im;     // the image forms' point source (data null: `points`)
};
void scan_consts(const fpe_scan_params& sp, const fpe_scan& scan, const MapGeom& g, ScanArgs& a);  // fpe_host.cpp
// The descriptor as the kernels take it, with the three device addresses (fpe_host.cpp)
void scan_image_consts(const fpe_scan_image& im, const void* d_image, const float* d_rowDir, const float* d_colDir, ScanImage& out);
// The three passes of a fuse on `stream`, and each alone.  merge: the merged form of the two point passes.
hipError_t launch_scan_fuse(const ScanArgs& a, bool merge, hipStream_t stream);
hipError_t launch_scan_top(const ScanArgs& a, bool merge, hipStream_t stream);
hipError_t launch_scan_sum(const ScanArgs& a, bool merge, hipStream_t stream);
hipError_t launch_scan_cells(const ScanArgs& a, hipStream_t stream);
// The image forms' fuse (a.im.data set; fpe_scan_image.hpp): scan_top_image_kernel, then the merged sum pass and the cell pass.
hipError_t launch_scan_fuse_image(const ScanArgs& a, hipStream_t stream);
hipError_t launch_scan_top_image(const ScanArgs& a, hipStream_t stream);
// every cell's scratch and the accumulators to their rest values (create)
hipError_t launch_scan_reset(ScanCell* cells, size_t n, int32_t* acc, hipStream_t stream);
// new (i, j) = old (i + sr, j + sc) of both layers, or the cleared value (|sr| <= rows, |sc| <= cols: clamped by the caller)
hipError_t launch_scan_move(const uint32_t* srcElev, const uint32_t* srcVar, uint32_t* dstElev, uint32_t* dstVar, int rows, int cols, int sr, int sc,
                            hipStream_t stream);
// both layers from two sources: a cell that is NaN in either becomes the cleared value in both (srcElev null: every cell cleared)
hipError_t launch_scan_set(const uint32_t* srcElev, const uint32_t* srcVar, uint32_t* dstElev, uint32_t* dstVar, size_t n, hipStream_t stream);

// ---- scan visibility clearing (fpe_scan_clear.hpp) -------------------------------------------------------------
// The clear shares the state's scratch with the fuse (the two never overlap on one state): a cell's hits are counted in ScanCell's
// `count` word (0 at rest), the bounding box and the ticket are the fuse's accumulator words 12-15 and 16 (same rest values), and
// its own totals live in words the fuse leaves at 0:
constexpr int kClearAccDropped = 17;  // then rays, rays_long, rays_empty, cells_hit, cells_cleared: fpe_scan_clear_info's words 2-7
constexpr int kClearAccWide = 24;     // samples_in_roi and hit_pairs, 64 bits each (words 24-27; 8-byte aligned): the info's words 12-15
// The argument block of both passes, by value.
struct ScanClearArgs {
    double T[12];
    double minR2, maxR2, minZ, maxZ;
    MapGeom g;
    double step;        // double(sample_step) * resolution
    double margin;      // double(margin)
    double maxSamples;  // double(max_samples)
    int32_t startSamples, endSamples, minHits, rayStride;
    int32_t n, stride;  // points, floats per point
    int32_t nCast;      // points that cast a ray or are dropped: ceil(n / rayStride)
    int32_t row0, col0, nr, nc;
    const float* points;
    ScanCell* cells;
    int32_t* acc;
    uint32_t* elev;
    uint32_t* var;
    int32_t* info;  // the caller's fpe_scan_clear_info (device) as sixteen words, or null
    ScanImage im;   // the image forms' point source (data null: `points`)
};
void scan_clear_consts(const fpe_scan_params& sp, const fpe_scan_clear_params& cp, const fpe_scan& scan, const MapGeom& g, ScanClearArgs& a);  // fpe_host.cpp
// The ray pass (form 1: one lane per ray; 2: `group` = 16, 32 or 64 adjacent lanes per ray) and the cell pass on `stream`.
hipError_t launch_scan_clear(const ScanClearArgs& a, int form, int group, hipStream_t stream);
hipError_t launch_scan_clear_rays(const ScanClearArgs& a, int form, int group, hipStream_t stream);
hipError_t launch_scan_clear_cells(const ScanClearArgs& a, hipStream_t stream);
// The image forms' clear (a.im.data set; fpe_scan_image.hpp): the same ray kernels with the pixel source, then the cell pass.
hipError_t launch_scan_clear_image(const ScanClearArgs& a, int form, int group, hipStream_t stream);

// ---- scan gap closing (fpe_scan_close.hpp) ---------------------------------------------------------------------
// The close has an accumulator block of its own (allocated with the state's `closed` layer, reset there): words 0-4 count the known,
// filled, no_support, rejected_axes and rejected_spread cells (at rest 0), words 8-11 are the filled cells' bounding box (at rest
// INT32_MAX, INT32_MAX, -1, -1), word 16 is the ticket (at rest 0); words 32-47 are the host forms' device info.
constexpr int kCloseAccWords = 48;
constexpr int kCloseAccBox = 8;
constexpr int kCloseTicket = 16;
constexpr int kCloseAccInfo = 32;
constexpr int kCloseMaxReach = 8;
// The argument block of the one launch, by value.
struct ScanCloseArgs {
    int32_t rows, cols;          // the state's size
    int32_t row0, col0, nr, nc;  // the rectangle
    int32_t reach, maxGap, minAxes;
    float maxSpread;
    int64_t outStride;     // floats (and bytes of cls) per output row
    const uint32_t* elev;  // the state's elevation, as 32-bit patterns: read only
    uint32_t* out;         // rectangle-local
    uint8_t* cls;          // rectangle-local, or null
    int32_t* acc;          // [kCloseAccWords]
    int32_t* info;         // the caller's fpe_scan_close_info (device) as sixteen words, or null
};
void scan_close_consts(const fpe_scan_close_params& kp, const int32_t rect[4], int rows, int cols, ScanCloseArgs& a);  // fpe_host.cpp
// One launch on `stream`.  form 1: direct, one lane per cell; 2: tiled, a 16 x 64 tile and its halo in LDS per workgroup.
hipError_t launch_scan_close(const ScanCloseArgs& a, int form, hipStream_t stream);
// the accumulator block to its rest values (when it is allocated)
hipError_t launch_scan_close_reset(int32_t* acc, hipStream_t stream);

}  // namespace fpe
