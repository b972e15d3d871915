// fpe_host.hpp — host-side logic of the engine that needs no GPU: parameter typing, derived
// constants, the spiral rank table, tile sizing, GlobalFootholds message assembly, and what the filter chain and an
// elevation-driven map update launch (filter_route, plan_elevation_update).
#pragma once
#include <cstdint>
#include <vector>

#include "fpe_launch.hpp"

namespace fpe {

// Upper bound of SpiralIterator rings the rank table is built for (ceil(R/res) must not exceed it).
constexpr int kMaxRings = 96;

struct SpiralTable {
    std::vector<int16_t> di, dj;
    std::vector<uint8_t> ring;
    std::vector<int32_t> ringStart;  // [nRings + 2]
    int maxRing = 0;
};
// SpiralIterator visiting order for rings 0..nRings as index offsets from the centre cell
// (grid_map SpiralIterator::generateRing; consumed from the back — SURVEY.md App. A.5).
void build_spiral_table(int nRings, SpiralTable& out);

// initialize() constants with the reference's float/double typing (cpp:340-421, 2693).
void derive_constants(const fpe_params& p, const MapGeom& g, float maxSearchRadius, const Tuning& tuning, PlanConsts& out);

// Offsets of a cell-centred disc of radius double(footRadius) and the proof that they are
// rounding-robust on this map (see PlanConsts::footRobust).
void derive_foot_offsets(float footRadius, const MapGeom& g, PlanConsts& out);

// Tile half-width (cells) that covers: every spiral candidate's foot disc, the default disc and
// the centroid rectangle for search radii up to maxSearchRadius.
int tile_halfwidth(float maxSearchRadius, float footRadius, double resolution);

// Half-width of the window that provably contains every cell a leg search can touch (bit-window kernels), or 0
// when one of the proofs those kernels rest on does not hold for these parameters on this map.
int bits_window_halfwidth(const PlanConsts& c, const MapGeom& g);

// number of rings ceil(double(R)/res) as SpiralIterator computes it
int spiral_rings(float searchRadius, double resolution);

int validate_params(const fpe_params& p);

// The refusals of fpe_update_map* for a map of rows x cols cells (include/fpe.h): FPE_OK, or FPE_E_INVALID_ARG with *why set.
// elevationOnly: the patches of fpe_update_elevation* (elevation required, traversability must be null).
int check_map_update(int rows, int cols, const fpe_map_update* u, bool elevationOnly, const char** why);
// Size and resolution of a map the engine takes (fpe_upload_map*, fpe_traversability*, fpe_update_elevation*): FPE_OK, or
// FPE_E_INVALID_ARG with *why set.
int check_map_geometry(int rows, int cols, double res, const char** why);
// The refusals of fpe_scan_fuse* for a state of rows x cols cells (include/fpe.h): FPE_OK, or FPE_E_INVALID_ARG with *why set.
int check_scan(int rows, int cols, const fpe_scan_params* sp, const fpe_scan* scan, const char** why);
void scan_params_defaults(fpe_scan_params& out);
// The refusals of fpe_scan_clear*: check_scan's, then the clear parameters'.
int check_scan_clear(int rows, int cols, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const char** why);
void scan_clear_params_defaults(fpe_scan_clear_params& out);
// The refusals of fpe_scan_close* for a state of rows x cols cells: the parameters' ranges, then the rectangle.
int check_scan_close(int rows, int cols, const fpe_scan_close_params* kp, const int32_t rect[4], const char** why);
void scan_close_params_defaults(fpe_scan_close_params& out);
// The refusals of the image forms (point 6 of the scan block): check_scan's (check_scan_clear's when cp is given), then the
// descriptor's, then scan->n_points against the selected pixels.
int check_scan_image(int rows, int cols, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const fpe_scan_image* im,
                     const char** why);
// The descriptor's own refusals (everything of the list that needs neither the state nor the scan)
int check_scan_image_desc(const fpe_scan_image* im, const char** why);
// The selected rows and columns of a valid descriptor.
inline int scan_image_sel_rows(const fpe_scan_image& im) { return (im.height - 1) / im.row_step + 1; }
inline int scan_image_sel_cols(const fpe_scan_image& im) { return (im.width - 1) / im.col_step + 1; }

// ---- the producer's filter chain (fpe_filters.hpp): its host arithmetic — filter_route and friends are declared in fpe_launch.hpp ----
void filter_params_defaults(fpe_filter_params& out);
// fpe_filter_params -> FilterConsts; FPE_E_INVALID_ARG for a radius or critical value that is not positive and finite.
int filter_consts(const fpe_filter_params& fp, FilterConsts& fc);
extern const char* const kBadFilterParams;  // the fpe_last_error text of that refusal
// What fpe_elevation_update_plan and the engine's fpe_update_elevation* share (host arithmetic only): the refusals, the new
// geometry, the clamped shift, the dirty set D as rectangles, the route and — route 0 — the tile rectangles of the region launches.
struct ElevationUpdatePlan {
    fpe_elevation_update_info info;
    FilterConsts fc;
    MapGeom g;
    FilterRoute rt;
    int sr, sc;
    std::vector<CellRect> dirty;
    FilterRegion region;
};
void elevation_dirty_rects(int rows, int cols, int R, int sr, int sc, const fpe_map_update* u, std::vector<CellRect>& out);
int plan_elevation_update(int rows, int cols, double res, const fpe_filter_params* fp, const fpe_map_update* u, ElevationUpdatePlan& plan, const char** why);


// Opt track: the file-scope NLopt globals (cpp:28-51, 497-498, 514), the constraint thresholds
// t1..t4 (cpp:1156-1159) and the column bounds of xBounds (cpp:1063-1066, 528-529), with the reference's typing.
// FPE_E_INVALID_ARG when a weight / scale / tolerance is not finite.
int derive_opt_constants(const fpe_params& p, const fpe_opt_params& op, const MapGeom& g, const PlanConsts& pc, OptConsts& out);

// GlobalFootholds message content from one pose's plan outputs (cpp:591-699, 1378-1396, 1574).
void assemble_global_footholds(const fpe_foothold* nominal, const uint8_t* cycleOk, const double* stance,
                               int nCycles, fpe_global_footholds* msg);
// centroidGlobalFootholdsMsg_ content of one call (cpp:709-727, 1444-1462): its own bookkeeping, not the nominal one
void assemble_centroid_footholds(const fpe_centroid_foothold* centroid, const uint8_t* cycleOk, const double* stance,
                                 int nCycles, fpe_global_footholds* msg);
void assemble_track_report(const double* resultXYZ, const uint8_t* cycleOk, const double* stance, int nCycles,
                           const fpe_params& params, fpe_track_report* rep);
// optGlobalFootholdsMsg_ content of one call (cpp:737-755, 1510-1532): bookkeeping as the centroid message
void assemble_opt_footholds(const fpe_opt_foothold* opt, const uint8_t* cycleOk, const double* stance, int nCycles,
                            fpe_global_footholds* msg);
// centroidFeetCenterPath as the reference fills it (cpp:792 and cpp:946): per cycle the centroid track's feet centre,
// then the opt track's
void interleave_centroid_path(fpe_track_report* centroid, const fpe_track_report& opt);

}  // namespace fpe
