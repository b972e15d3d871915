// fpe_host.cpp — host-side logic of the engine (no GPU calls in this file).
#include "fpe_host.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace fpe {

// ---- SpiralIterator visiting order ---------------------------------------------------------------
// grid_map SpiralIterator::generateRing walks ring d counter-clockwise from offset (d, 0), keeping
// to cells whose truncated Euclidean index distance equals d, and the iterator then pops cells from
// the BACK of the ring vector; so ring d is visited in the reverse of the walk.
// The table holds the unfiltered order; the in-map test and the in-radius test of the last two
// rings only remove entries, they never reorder (fpe_kernels.hip::candidate_search_wave).
namespace {
inline int sgn(int v) { return (v > 0) - (v < 0); }
inline int trunc_norm(int x, int y) {
    return static_cast<int>(std::sqrt(static_cast<double>(x) * x + static_cast<double>(y) * y));
}
}  // namespace

void build_spiral_table(int nRings, SpiralTable& out) {
    out.di.clear();
    out.dj.clear();
    out.ring.clear();
    out.ringStart.assign(1, 0);
    out.maxRing = nRings;
    out.di.push_back(0);
    out.dj.push_back(0);
    out.ring.push_back(0);
    std::vector<std::pair<int, int>> walk;
    for (int d = 1; d <= nRings; ++d) {
        out.ringStart.push_back(static_cast<int32_t>(out.di.size()));
        walk.clear();
        int px = d, py = 0;
        do {
            walk.emplace_back(px, py);
            const int nx = -sgn(py), ny = sgn(px);
            if (nx != 0 && trunc_norm(px + nx, py) == d) {
                px += nx;
            } else if (ny != 0 && trunc_norm(px, py + ny) == d) {
                py += ny;
            } else {
                px += nx;
                py += ny;
            }
        } while (px != d || py != 0);
        for (auto it = walk.rbegin(); it != walk.rend(); ++it) {
            out.di.push_back(static_cast<int16_t>(it->first));
            out.dj.push_back(static_cast<int16_t>(it->second));
            out.ring.push_back(static_cast<uint8_t>(d));
        }
    }
    out.ringStart.push_back(static_cast<int32_t>(out.di.size()));  // end sentinel = ringStart[nRings+1]
}

int spiral_rings(float searchRadius, double resolution) {
    const double R = static_cast<double>(searchRadius);
    return static_cast<int>(static_cast<unsigned int>(std::ceil(R / resolution)));
}

int tile_halfwidth(float maxSearchRadius, float footRadius, double resolution) {
    const double R = static_cast<double>(maxSearchRadius);
    const double rf = static_cast<double>(footRadius);
    const int nRings = static_cast<int>(std::ceil(R / resolution));
    const int nFootBox = static_cast<int>(std::ceil(rf / resolution)) + 1;  // bbox of a disc around any point
    // candidates reach nRings cells from the centre index and their discs nFootBox further; the
    // centroid rectangle reaches ceil(R/res)+1 rows; +1 guards the continuous-centre offset
    return nRings + nFootBox + 1;
}

// The bit-window kernels (fpe_bits.hpp) look every traversability decision up in a window of row masks around
// getIndex(centre).  They are exact when
//  (1) the foot-disc offset table is proved (derive_foot_offsets) and has at most 64 entries (one per lane of the
//      widest kernel; the 8-lane kernels take up to 32: fpe_bits.hpp::bits_supported);
//  (2) every cell a search can touch lies within `H` cells of the centre index.  For a bounded position p and the
//      centre c the index difference is floor-like in (p - c) / res; with rounding errors of at most `slack` cells
//      (positions are rewritten by boundPositionToRange and divided by res in f64) the reach of an extent d is
//      floor(d / res + frac) <= ceil(d / res) cells, one more when d / res is within `slack` of an integer.
//      Extents: the centroid rectangle reaches R rows (lx / 2 = R) and R / 2 columns (cpp:1616-1617); a spiral
//      candidate of an unfiltered ring lies within nRings - 2 cells, one of the two filtered rings has its cell
//      centre within R of the continuous centre (SpiralIterator::isInside), i.e. at most floor(R / res + 1/2) cells
//      from the centre cell, and its foot disc footReach further; a member of the centre's own disc at most
//      floor(rf / res + 1/2) cells;
//  (3) getIndex(cell centre of the centroid submap) is the top-left index plus (row, col): the submap's cell centres
//      differ from the map's by a few ulps of the coordinate magnitude, which must be far below half a cell;
//  (4) index predictions (base - limit) / res fit an int with room to spare.
// Search centres outside the map need no extra room: their clamped boxes hold no disc member and getSubmap fails.
int bits_window_halfwidth(const PlanConsts& c, const MapGeom& g) {
    if (!c.footRobust || c.nFoot < 1 || c.nFoot > 64) return 0;
    const double res = g.res;
    const double R = static_cast<double>(c.maxSearchRadius), rf = c.rf;
    const double mag = std::fabs(g.posX) + g.lenX + std::fabs(g.posY) + g.lenY + R + rf + 1.0;
    const double slack = 64.0 * DBL_EPSILON * mag / res + 1e-12;  // rounding error of an index quotient, in cells
    if (!(slack < 1e-3)) return 0;                                 // (3): also keeps cell centres far from cell edges
    if (!((mag + 2.0e6) / res < 5.0e8)) return 0;                  // (4)
    if (!(R / res < 1.0e4) || !(rf / res < 1.0e3)) return 0;
    auto reach = [&](double d) {  // rows between getIndex(centre) and getIndex(centre +- d): ceil(d / res), one more on a tie
        const double q = d / res;
        int n = static_cast<int>(std::ceil(q));
        if (std::fabs(q - std::round(q)) <= slack) n = static_cast<int>(std::round(q)) + 1;
        return n;
    };
    auto within = [&](double d) {  // largest index offset of a cell CENTRE within d of a point of the centre cell
        return static_cast<int>(std::floor((d + 0.5 * res) / res + slack));
    };
    const int nRings = spiral_rings(c.maxSearchRadius, res);
    const int rectReach = reach(R);
    // a candidate of the two filtered rings has its cell centre within R of the continuous centre, which lies within
    // half a cell of the centre cell's centre; unfiltered rings end at nRings - 2
    const int candReach = std::min(nRings, std::max(nRings - 2, within(R))) + c.footReach;
    const int discReach = within(rf);  // members of the continuous-centre disc
    return std::max(std::max(rectReach, candReach), std::max(discReach, 1));
}

int validate_params(const fpe_params& p) {
    const float fs[] = {p.footRadius, p.defaultFootholdThreshold, p.candidateFootholdThreshold, p.searchRadius,
                        p.stepLength, p.length, p.width, p.l1, p.skew};
    for (float f : fs)
        if (!std::isfinite(f)) return FPE_E_INVALID_ARG;
    if (!(p.footRadius >= 0.0f) || !(p.searchRadius >= 0.0f)) return FPE_E_INVALID_ARG;
    if (!std::isfinite(p.h) || !std::isfinite(p.lateralDrift)) return FPE_E_INVALID_ARG;
    return FPE_OK;
}

// initialize(), cpp:340-421.  lengthBase / widthBase / skew / stepLength_ are float members
// (hpp:657-668, 683, 613); widthBase is computed in f32 (cpp:341); each use below promotes the
// float operand to double exactly where the reference's expression does.
// A cell-centred CircleIterator visits cell q = candidate + (a, b) iff the f64 expression
// dx*dx + dy*dy <= rf*rf holds, with dx = cell_pos(i+a) - cell_pos(i).  In exact
// arithmetic that is (a^2 + b^2) res^2 <= rf^2, independent of the candidate.  The f64 evaluation
// differs from the exact value by at most `tol` (two rounded cell positions of magnitude <= |P|+L
// per axis, then squares and a sum), so when every lattice offset near the circle clears the radius
// by more than tol the visited set is the same offset list for every candidate, and the
// iterator's bounding box (>= half a cell of slack) always contains it.  Otherwise footRobust = 0
// and the kernels walk the literal per-candidate bounding box.
void derive_foot_offsets(float footRadius, const MapGeom& g, PlanConsts& c) {
    const double rf = static_cast<double>(footRadius);
    const double res = g.res;
    const double rf2 = rf * rf;
    const double maxAbs = std::max(std::fabs(g.posX) + g.lenX, std::fabs(g.posY) + g.lenY) + rf + res;
    const double e1 = 4.0 * maxAbs * DBL_EPSILON;                    // |error| of one position difference
    const double tol = 4.0 * (rf + 2.0 * res) * e1 + 1e-9 * rf2 + 8.0 * DBL_EPSILON * rf2;
    const int reach = static_cast<int>(std::ceil(rf / res)) + 1;
    c.nFoot = 0;
    c.footRobust = 1;
    c.footReach = reach;  // bound of the literal bounding-box walk; tightened below when the table is valid
    if (reach > 100) {
        c.footRobust = 0;
        return;
    }
    for (int a = -reach; a <= reach; ++a)
        for (int b = -reach; b <= reach; ++b) {
            const double d2 = (static_cast<double>(a) * a + static_cast<double>(b) * b) * (res * res);
            if (std::fabs(d2 - rf2) <= tol) {
                c.footRobust = 0;  // a lattice point sits on the circle within rounding: stay literal
                c.nFoot = 0;
                return;
            }
            if (d2 < rf2) {
                if (c.nFoot >= kMaxFootOffsets) {
                    c.footRobust = 0;
                    c.nFoot = 0;
                    return;
                }
                c.footDa[c.nFoot] = static_cast<int8_t>(a);
                c.footDb[c.nFoot] = static_cast<int8_t>(b);
                ++c.nFoot;
            }
        }
    int mx = 0;
    for (int k = 0; k < c.nFoot; ++k) mx = std::max(mx, std::max(std::abs(static_cast<int>(c.footDa[k])), std::abs(static_cast<int>(c.footDb[k]))));
    c.footReach = mx;
    // Row-interval form of the table: a disc's row +-a holds the columns [-w(a), w(a)].  Verified entry by entry, so
    // the kernels may erode with one interval per row instead of one shift per offset.
    c.nHW = 0;
    if (mx <= 15) {
        int w[16];
        for (int a = 0; a < 16; ++a) w[a] = -1;
        for (int k = 0; k < c.nFoot; ++k) w[std::abs(static_cast<int>(c.footDa[k]))] = std::max(w[std::abs(static_cast<int>(c.footDa[k]))], std::abs(static_cast<int>(c.footDb[k])));
        int expect = 0;
        bool ok = true;
        for (int a = 0; a <= mx; ++a) {
            if (w[a] < 0) ok = false;
            else expect += (a == 0 ? 1 : 2) * (2 * w[a] + 1);
            if (a > 0 && w[a] > w[a - 1]) ok = false;  // (the kernels' nested erosion takes the widths in non-increasing order)
        }
        if (ok && expect == c.nFoot) {  // |set| matches and every entry lies inside its row interval: the forms are equal
            int n = 0;
            for (int a = 0; a <= mx && ok; ++a) {
                int idx = -1;
                for (int q = 0; q < n; ++q)
                    if (c.hwList[q] == w[a]) idx = q;
                if (idx < 0) {
                    if (n >= kMaxHW) {
                        ok = false;
                        break;
                    }
                    c.hwList[n] = static_cast<int8_t>(w[a]);
                    idx = n++;
                }
                c.hwIdx[a] = static_cast<int8_t>(idx);
            }
            if (ok) c.nHW = n;
        }
    }
}

void derive_constants(const fpe_params& p, const MapGeom& geom, float maxSearchRadius, const Tuning& tuning, PlanConsts& c) {
    const double resolution = geom.res;
    std::memset(&c, 0, sizeof(c));
    c.footRadius = p.footRadius;
    c.thrDefault = p.defaultFootholdThreshold;
    c.thrCandidate = p.candidateFootholdThreshold;
    c.searchRadius = p.searchRadius;
    c.rf = static_cast<double>(p.footRadius);
    c.rf2 = c.rf * c.rf;  // CircleIterator: radiusSquare_ = pow(radius_, 2)
    const float lengthBase = p.length;           // cpp:340
    const float widthBase = p.width + p.l1 * 2;  // cpp:341
    c.LbHalf = lengthBase * 0.5;                 // cpp:350
    c.WbHalfNeg = -widthBase * 0.5;              // cpp:351
    c.WbHalfPos = widthBase * 0.5;               // cpp:359
    const double k = static_cast<double>(p.skew);
    // cpp:403-421: RF_FIRST flips the sign of skew
    c.biasX[0] = p.RF_FIRST ? 0.5 * lengthBase + k : 0.5 * lengthBase - k;     // RF
    c.biasX[1] = p.RF_FIRST ? -0.5 * lengthBase - k : -0.5 * lengthBase + k;   // RH
    c.biasX[2] = p.RF_FIRST ? -0.5 * lengthBase + k : -0.5 * lengthBase - k;   // LH
    c.biasX[3] = p.RF_FIRST ? 0.5 * lengthBase - k : 0.5 * lengthBase + k;     // LF
    c.biasY[0] = -0.5 * widthBase;
    c.biasY[1] = -0.5 * widthBase;
    c.biasY[2] = 0.5 * widthBase;
    c.biasY[3] = 0.5 * widthBase;
    c.stepHalf = p.stepLength / 2;     // cpp:2693 (float / int)
    c.step = p.stepLength;             // cpp:2199
    c.stepQuarter = p.stepLength / 4;  // build-defined walk gait
    c.h = p.h;
    c.drift = p.lateralDrift;
    c.RF_FIRST = p.RF_FIRST ? 1 : 0;
    c.maxSearchRadius = maxSearchRadius;
    c.tileH = tile_halfwidth(maxSearchRadius, p.footRadius, resolution);
    {
        // the per-leg LDS tile (tileW^2 flag bytes + 16 tileW of column crossings, fpe_kernels.hip::tile_total_bytes)
        // doubles as float scratch of the ordered height sums, one float per visited cell of a foot-disc bounding
        // box of up to (2 ceil(rf/res) + 2)^2 cells: a foot radius much larger than the search radius must not
        // overrun it, so the tile grows until the scratch fits
        const double boxSide = 2.0 * std::ceil(c.rf / resolution) + 2.0;
        const double scratch = 4.0 * boxSide * boxSide;
        while (static_cast<double>(2 * c.tileH + 1) * (2 * c.tileH + 1) + 16.0 * (2 * c.tileH + 1) < scratch && c.tileH < 4096) ++c.tileH;
    }
    c.tileW = 2 * c.tileH + 1;
    c.tileWMagic = fastdiv_magic(static_cast<uint32_t>(c.tileW));
    c.groupOverride = tuning.planGroup;
    c.noMidVariant = tuning.noMidVariant;
    c.noBits = tuning.noBits;
    c.reserved = 0;
    // isos_ (cpp:384-394): longEdge = lengthBase + skew*2 in f32 (hpp:666, 683), promoted on assignment to the
    // double member (hpp:679); footSearchRect_.length = searchRadius_*2 and .width = searchRadius_ are f32 values
    // stored in doubles (hpp:700-701); the sums are f64
    {
        const float longEdgeF = lengthBase + p.skew * 2;
        const double longEdge = longEdgeF, shortEdge = widthBase;
        const double rectLen = p.searchRadius * 2, rectWid = p.searchRadius;
        c.isosLen = longEdge + rectLen;
        c.isosWid = shortEdge + rectWid;
    }
    derive_foot_offsets(p.footRadius, geom, c);
    // Middle cell of an unclamped 3x3 CircleIterator box.  The box rows are i0 = index(cx + r) .. i0 + 2 =
    // index(cx - r) (findSubmapParameters); cell i covers (x_i - res/2, x_i + res/2], so cx + r <= x_m + 1.5 res and
    // cx - r >= x_m - 1.5 res for the middle row's centre x_m, i.e. |cx - x_m| <= 1.5 res - r, and likewise in y.
    // With r >= 0.9 res the middle cell's squared distance is <= 2 (0.6 res)^2 = 0.72 res^2 < 0.81 res^2 <= r^2: an 11 %
    // margin against rounding errors of order 1e-9 m (|coordinates| <= 1e6), so the reference's f64 test
    // dx*dx + dy*dy <= r^2 is true for that cell without evaluating it.
    c.midCellInside = (c.rf >= 0.9 * resolution) ? 1 : 0;
    if (tuning.literalDiscs) {
        c.midCellInside = 0;
        c.footRobust = 0;
        c.footReach = static_cast<int>(std::ceil(c.rf / resolution)) + 1;
    }  // test knob: force the literal bounding-box walk
    c.winH = bits_window_halfwidth(c, geom);
    {
        // bound of the rounding error of an index quotient, in cells (the same bound as `slack` above, doubled)
        const double mag = std::fabs(geom.posX) + geom.lenX + std::fabs(geom.posY) + geom.lenY +
                           static_cast<double>(maxSearchRadius) + c.rf + 1.0;
        c.cornerEps = 128.0 * DBL_EPSILON * mag / resolution + 1e-12;
    }
}

// globalFootholdPlan message bookkeeping: cpp:681-699 (stance entries), cpp:1378-1396 (valid
// cycle), cpp:1574 (invalid cycle: success=false, nothing appended).
void assemble_global_footholds(const fpe_foothold* nominal, const uint8_t* cycleOk, const double* stance,
                               int nCycles, fpe_global_footholds* msg) {
    std::memset(msg, 0, sizeof(*msg));
    msg->gait_cycles = static_cast<uint8_t>(nCycles);
    msg->gait_cycles_succeed = 0;
    msg->success = 0;
    int n = 0;
    for (int l = 0; l < 4; ++l) {
        fpe_msg_foothold& f = msg->footholds[n++];
        f.x = stance[l * 3 + 0];
        f.y = stance[l * 3 + 1];
        f.z = stance[l * 3 + 2];
        f.foot_id = static_cast<uint8_t>(l);
        f.gait_cycle_id = 0;
    }
    for (int g = 0; g < nCycles; ++g) {
        if (cycleOk[g]) {
            msg->gait_cycles_succeed = static_cast<uint8_t>(g + 1);
            msg->success = 1;
            for (int l = 0; l < 4; ++l) {
                const fpe_foothold& s = nominal[g * 4 + l];
                fpe_msg_foothold& f = msg->footholds[n++];
                f.x = s.x;
                f.y = s.y;
                f.z = static_cast<double>(s.z);
                f.foot_id = static_cast<uint8_t>(l);
                f.gait_cycle_id = static_cast<uint8_t>(g);
            }
        } else {
            msg->success = 0;
        }
    }
    msg->n_footholds = n;
}

// centroidGlobalFootholdsMsg_ (cpp:709-727, 1444-1462).  Unlike the nominal message its `success` is set false
// once per call (cpp:711) and true on every committed cycle (cpp:1446) — a failed cycle never clears it again
// (cpp:1574 touches nominalGlobalFootholdsMsg_ only) — and its `gait_cycles` field is never written (stays 0).
void assemble_centroid_footholds(const fpe_centroid_foothold* cen, const uint8_t* cycleOk, const double* stance,
                                 int nCycles, fpe_global_footholds* msg) {
    std::memset(msg, 0, sizeof(*msg));
    int n = 0;
    for (int l = 0; l < 4; ++l) {
        fpe_msg_foothold& f = msg->footholds[n++];
        f.x = stance[l * 3 + 0];
        f.y = stance[l * 3 + 1];
        f.z = stance[l * 3 + 2];
        f.foot_id = static_cast<uint8_t>(l);
        f.gait_cycle_id = 0;
    }
    for (int g = 0; g < nCycles; ++g) {
        if (!cycleOk[g]) continue;
        msg->gait_cycles_succeed = static_cast<uint8_t>(g + 1);  // cpp:1445
        msg->success = 1;                                        // cpp:1446
        for (int l = 0; l < 4; ++l) {
            const fpe_centroid_foothold& s = cen[g * 4 + l];
            fpe_msg_foothold& f = msg->footholds[n++];
            f.x = s.x;
            f.y = s.y;
            f.z = static_cast<double>(s.z);
            f.foot_id = static_cast<uint8_t>(l);
            f.gait_cycle_id = static_cast<uint8_t>(g);
        }
    }
    msg->n_footholds = n;
}

// getPolygonCenter (cpp:2421-2463) on the host, with z (= mean of the four z, cpp:2459-2461).
static void polygon_center_host(const double feet[4][3], double out[3]) {
    const double x1 = feet[0][0], y1 = feet[0][1];
    double x2 = feet[1][0], y2 = feet[1][1];
    double sum_x = 0, sum_y = 0, sum_s = 0;
    for (int i = 1; i <= 2; i++) {
        const double x3 = feet[i + 1][0], y3 = feet[i + 1][1];
        const double s = ((x2 - x1) * (y3 - y1) - (x3 - x1) * (y2 - y1)) / 2.0;
        sum_x += (x1 + x2 + x3) * s;
        sum_y += (y1 + y2 + y3) * s;
        sum_s += s;
        x2 = x3;
        y2 = y3;
    }
    out[0] = sum_x / sum_s / 3.0;
    out[1] = sum_y / sum_s / 3.0;
    out[2] = (feet[0][2] + feet[1][2] + feet[2][2] + feet[3][2]) / 4.0;
}

// Feet-centre path and KPIs of one track, rebuilt from the kernel's per-cycle results: the track's
// current feet start at the stance shifted by -stepLength_/2 (setFirstGait, cpp:2679-2699) and take the
// results of every committed cycle (cpp:1413-1416 / 1480-1483).
void assemble_track_report(const double* resultXYZ /*[nCycles][4][3]*/, const uint8_t* cycleOk, const double* stance,
                           int nCycles, const fpe_params& params, fpe_track_report* rep) {
    std::memset(rep, 0, sizeof(*rep));
    const double stepHalf = static_cast<double>(params.stepLength / 2);
    double cur[4][3];
    for (int l = 0; l < 4; ++l) {
        cur[l][0] = stance[l * 3 + 0] - stepHalf;
        cur[l][1] = stance[l * 3 + 1];
        cur[l][2] = stance[l * 3 + 2];
    }
    enum { RF = 0, RH = 1, LH = 2, LF = 3 };
    const double gaitCycle = 1.0;  // cpp:332
    for (int g = 0; g < nCycles; ++g) {
        polygon_center_host(cur, rep->feet_center_path[rep->n_path++]);
        if (!cycleOk[g]) continue;
        const double(*r)[3] = reinterpret_cast<const double(*)[3]>(resultXYZ + static_cast<size_t>(g) * 12);
        rep->feet_distance[rep->n_kpi] = r[RF][0] - r[LH][0];
        rep->feet_distance[rep->n_kpi + 1] = r[LF][0] - r[RH][0];
        double c1, c2, c3;
        if (params.RF_FIRST) {
            c1 = (cur[RF][0] + cur[LH][0]) / 2;
            c2 = (r[LF][0] + r[RH][0]) / 2;
            c3 = (r[RF][0] + r[LH][0]) / 2;
        } else {
            c1 = (cur[LF][0] + cur[RH][0]) / 2;
            c2 = (r[RF][0] + r[LH][0]) / 2;
            c3 = (r[LF][0] + r[RH][0]) / 2;
        }
        const double d1 = c2 - c1, d2 = c3 - c2;
        rep->cog_speed[rep->n_kpi] = d1 / (0.5 * gaitCycle);
        rep->cog_speed[rep->n_kpi + 1] = d2 / (0.5 * gaitCycle);
        rep->n_kpi += 2;
        for (int l = 0; l < 4; ++l)
            for (int k = 0; k < 3; ++k) cur[l][k] = r[l][k];
    }
}

int derive_opt_constants(const fpe_params& p, const fpe_opt_params& op, const MapGeom& g, const PlanConsts& pc, OptConsts& oc) {
    const double vals[] = {op.w1, op.w2, op.w3, op.w4, op.wr, op.wc, op.ctol, op.hip_lower_scale, op.hip_upper_scale,
                           op.skew_lower_scale, op.skew_upper_scale, op.lf_current_row0, op.rh_current_row0};
    for (double v : vals)
        if (!std::isfinite(v)) return FPE_E_INVALID_ARG;
    oc.w1 = op.w1; oc.w2 = op.w2; oc.w3 = op.w3; oc.w4 = op.w4; oc.wr = op.wr; oc.wc = op.wc;
    oc.ctol = op.ctol;
    const double lengthBase = static_cast<double>(p.length);  // cpp:497: lengthBase = laikagoKinematics_.lengthBase (float)
    const double skew = static_cast<double>(p.skew);          // cpp:498
    const double mapResolution = g.res;                       // cpp:514
    oc.lengthBase = lengthBase;
    oc.skew = skew;
    oc.mapResolution = mapResolution;
    const double hip_lower_scale = op.hip_lower_scale, hip_upper_scale = op.hip_upper_scale;
    const double skew_lower_scale = op.skew_lower_scale, skew_upper_scale = op.skew_upper_scale;
    oc.t1 = lengthBase * hip_lower_scale/mapResolution;   // cpp:1156
    oc.t2 = lengthBase * hip_upper_scale/mapResolution;   // cpp:1157
    oc.t3 = 2* skew * skew_lower_scale/mapResolution;     // cpp:1158
    oc.t4 = 2* skew * skew_upper_scale/mapResolution;     // cpp:1159
    oc.lbOverRes = lengthBase/mapResolution;              // cpp:69-70
    oc.skew2OverRes = 2*skew/mapResolution;               // cpp:71-72
    oc.lfRow0 = op.lf_current_row0;
    oc.rhRow0 = op.rh_current_row0;
    oc.useConstraints = op.use_inequality_constraints ? 1 : 0;
    // footSearchRect_.width = searchRadius_ (an f32 value in a double, cpp:385); .col = width / mapResolution, a double
    // (cpp:529, hpp:704-705); Eigen::MatrixXi assignments truncate toward zero (cpp:1063-1066)
    const double footSearchRectWidth = p.searchRadius;
    const double footSearchRectCol = footSearchRectWidth/mapResolution;
    const double a = footSearchRectCol, b = pc.isosWid/mapResolution - footSearchRectCol, c = pc.isosWid/mapResolution;
    if (!(std::fabs(a) < 2.0e9) || !(std::fabs(b) < 2.0e9) || !(std::fabs(c) < 2.0e9)) return FPE_E_INVALID_ARG;
    oc.colLoA = 0;
    oc.colUpA = static_cast<int>(a);
    oc.colLoB = static_cast<int>(b);
    oc.colUpB = static_cast<int>(c);
    oc.pad = 0;
    return FPE_OK;
}

void assemble_opt_footholds(const fpe_opt_foothold* opt, const uint8_t* cycleOk, const double* stance, int nCycles,
                            fpe_global_footholds* msg) {
    std::memset(msg, 0, sizeof(*msg));
    int n = 0;
    for (int l = 0; l < 4; ++l) {  // cpp:737-755: the initial stance, gait_cycle_id 0
        fpe_msg_foothold& f = msg->footholds[n++];
        f.x = stance[l * 3 + 0];
        f.y = stance[l * 3 + 1];
        f.z = stance[l * 3 + 2];
        f.foot_id = static_cast<uint8_t>(l);
        f.gait_cycle_id = 0;
    }
    for (int g = 0; g < nCycles; ++g) {
        if (!cycleOk[g]) continue;
        msg->gait_cycles_succeed = static_cast<uint8_t>(g + 1);  // cpp:1511
        msg->success = 1;                                        // cpp:1512
        for (int l = 0; l < 4; ++l) {
            const fpe_opt_foothold& s = opt[g * 4 + l];
            fpe_msg_foothold& f = msg->footholds[n++];
            f.x = s.x;
            f.y = s.y;
            f.z = static_cast<double>(s.z);
            f.foot_id = static_cast<uint8_t>(l);
            f.gait_cycle_id = static_cast<uint8_t>(g);
        }
    }
    msg->n_footholds = n;
}

void interleave_centroid_path(fpe_track_report* cen, const fpe_track_report& opt) {
    const int n = cen->n_path < opt.n_path ? cen->n_path : opt.n_path;
    for (int g = n - 1; g >= 0; --g) {
        for (int k = 0; k < 3; ++k) {
            const double c = cen->feet_center_path[g][k];
            cen->feet_center_path[2 * g][k] = c;
            cen->feet_center_path[2 * g + 1][k] = opt.feet_center_path[g][k];
        }
    }
    cen->n_path = 2 * n;
}

}  // namespace fpe

// ---- C ABI: host-only entry points -----------------------------------------------------------------
extern "C" {

int fpe_params_yaml(fpe_params* p) {  // foothold_planner/config/foothold_planner.yaml:10-64
    if (!p) return FPE_E_INVALID_ARG;
    p->footRadius = float(0.02);
    p->defaultFootholdThreshold = float(0.9);
    p->candidateFootholdThreshold = float(0.7);
    p->searchRadius = float(0.1);
    p->stepLength = float(0.18);
    p->length = float(0.4387);
    p->width = float(0.175);
    p->l1 = float(0.037);
    p->skew = float(0.04);
    p->RF_FIRST = 0;
    p->h = 0.01;
    p->lateralDrift = -0.007;
    return FPE_OK;
}

int fpe_params_code_defaults(fpe_params* p) {  // readParameters, cpp:255-290
    if (!p) return FPE_E_INVALID_ARG;
    p->footRadius = float(0.03);
    p->defaultFootholdThreshold = float(0.7);
    p->candidateFootholdThreshold = float(0.7);
    p->searchRadius = float(0.1);
    p->stepLength = float(0.2);
    p->length = float(0.4387);
    p->width = float(0.175);
    p->l1 = float(0.037);
    p->skew = float(0.1);
    p->RF_FIRST = 0;
    p->h = 0.01;
    p->lateralDrift = -0.007;
    return FPE_OK;
}

int fpe_opt_params_yaml(fpe_opt_params* p) {  // foothold_planner.yaml:53-63, FootholdPlanner.cpp:34, 48-49
    if (!p) return FPE_E_INVALID_ARG;
    std::memset(p, 0, sizeof(*p));
    p->w1 = p->w2 = p->w3 = p->w4 = 1.0;
    p->wr = p->wc = 1.0;
    p->use_inequality_constraints = 1;
    p->ctol = 1e-2;
    p->hip_lower_scale = 0.9;
    p->hip_upper_scale = 1.1;
    p->skew_lower_scale = 0.8;
    p->skew_upper_scale = 1.2;
    return FPE_OK;
}

int fpe_opt_params_code_defaults(fpe_opt_params* p) {  // readParameters, cpp:297-307
    const int rc = fpe_opt_params_yaml(p);
    if (rc == FPE_OK) p->use_inequality_constraints = 0;
    return rc;
}

int fpe_spiral_offsets(int32_t n_rings, int32_t* out, int32_t max_cells) {
    if (n_rings < 0 || n_rings > fpe::kMaxRings) return FPE_E_INVALID_ARG;
    fpe::SpiralTable t;
    fpe::build_spiral_table(n_rings, t);
    const int n = static_cast<int>(t.di.size());
    if (out)
        for (int k = 0; k < n && k < max_cells; ++k) {
            out[3 * k + 0] = t.di[k];
            out[3 * k + 1] = t.dj[k];
            out[3 * k + 2] = t.ring[k];
        }
    return n;
}

int fpe_tile_halfwidth(float search_radius, float foot_radius, double resolution) {
    if (!(resolution > 0.0)) return FPE_E_INVALID_ARG;
    return fpe::tile_halfwidth(search_radius, foot_radius, resolution);
}

double fpe_algorithmic_bytes_per_foothold(float search_radius, float foot_radius, double resolution) {
    const double R = static_cast<double>(search_radius), rf = static_cast<double>(foot_radius);
    const int nS = static_cast<int>(std::floor(R / resolution + 0.5));
    const int nF = static_cast<int>(std::floor(rf / resolution));
    const int W = 2 * (nS + nF) + 1;
    int nFoot = 0;  // cells of a cell-centred foot disc
    const int reach = nF + 1;
    for (int a = -reach; a <= reach; ++a)
        for (int b = -reach; b <= reach; ++b)
            if ((static_cast<double>(a * a + b * b)) * resolution * resolution <= rf * rf) ++nFoot;
    return 4.0 * W * W + 8.0 * nFoot + 16.0;
}

// The state a plan starts from when no state is given: the stance (cpp:350-378) shifted by setFirstGait (cpp:2679-2699) in all three
// tracks, with derive_constants' typing — what the kernels' stance prologue writes to PoseShared::cur.
int fpe_plan_state_from_pose(const fpe_params* params, const fpe_pose* pose, const fpe_stride* stride, fpe_plan_state* out) {
    if (!params || !pose || !out) return FPE_E_INVALID_ARG;
    const float step = stride ? stride->step_length : params->stepLength;
    if (!std::isfinite(step) || (stride && stride->reserved != 0)) return FPE_E_INVALID_ARG;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(pose->position[k]) || std::fabs(pose->position[k]) > 1e6) return FPE_E_INVALID_ARG;
    const float lengthBase = params->length;                    // cpp:340
    const float widthBase = params->width + params->l1 * 2;     // cpp:341
    const double LbHalf = lengthBase * 0.5, WbHalfNeg = -widthBase * 0.5, WbHalfPos = widthBase * 0.5;  // cpp:350, 351, 359
    const double stepHalf = static_cast<double>(step / 2);      // cpp:2693 (float / int)
    std::memset(out, 0, sizeof(*out));
    for (int leg = 0; leg < 4; ++leg) {
        double sx = (leg == 0 || leg == 3) ? LbHalf : -LbHalf;
        double sy = (leg <= 1) ? WbHalfNeg : WbHalfPos;
        sx += pose->position[0];
        sy += pose->position[1];
        for (int t = 0; t < 3; ++t) {
            out->feet[t][leg][0] = sx - stepHalf;
            out->feet[t][leg][1] = sy;
        }
    }
    return FPE_OK;
}

int fpe_plan_state_from_feet(const double feet_xy[4][2], double adjusted_y, int32_t cycle, fpe_plan_state* out) {
    if (!feet_xy || !out) return FPE_E_INVALID_ARG;
    if (!std::isfinite(adjusted_y) || cycle < 0 || cycle > 254) return FPE_E_INVALID_ARG;
    for (int leg = 0; leg < 4; ++leg)
        if (!std::isfinite(feet_xy[leg][0]) || !std::isfinite(feet_xy[leg][1])) return FPE_E_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    for (int t = 0; t < 3; ++t)
        for (int leg = 0; leg < 4; ++leg) {
            out->feet[t][leg][0] = feet_xy[leg][0];
            out->feet[t][leg][1] = feet_xy[leg][1];
        }
    out->adjusted_y = adjusted_y;
    out->cycle = cycle;
    return FPE_OK;
}

int fpe_map_update_validate(const fpe_map_desc* base, const fpe_map_update* u) {
    if (!base) return FPE_E_INVALID_ARG;
    const char* why = nullptr;
    return fpe::check_map_update(base->rows, base->cols, u, false, &why);
}

int fpe_filter_reach_cells(const fpe_filter_params* fp, double resolution) {
    fpe_filter_params def;
    if (!fp) {
        fpe::filter_params_defaults(def);
        fp = &def;
    }
    fpe::FilterConsts fc;
    if (!(resolution > 0.0) || !std::isfinite(resolution) || fpe::filter_consts(*fp, fc) != FPE_OK) return FPE_E_INVALID_ARG;
    return fpe::filter_reach_cells(fc, resolution);
}

int fpe_elevation_update_plan(const fpe_map_desc* base, const fpe_filter_params* fp, const fpe_map_update* u, fpe_elevation_update_info* info,
                              uint8_t* dirty) {
    if (!base) return FPE_E_INVALID_ARG;
    fpe::ElevationUpdatePlan plan;
    const char* why = nullptr;
    const int rc = fpe::plan_elevation_update(base->rows, base->cols, base->resolution, fp, u, plan, &why);
    if (rc != FPE_OK) return rc;
    if (info) *info = plan.info;
    if (dirty) {
        std::memset(dirty, 0, static_cast<size_t>(base->rows) * base->cols);
        for (const fpe::CellRect& r : plan.dirty)
            for (int i = r.r0; i < r.r1; ++i) std::memset(dirty + static_cast<size_t>(i) * base->cols + r.c0, 1, static_cast<size_t>(r.c1 - r.c0));
    }
    return FPE_OK;
}

int fpe_scan_params_defaults(fpe_scan_params* out) {
    if (!out) return FPE_E_INVALID_ARG;
    fpe::scan_params_defaults(*out);
    return FPE_OK;
}

int fpe_scan_validate(const fpe_map_desc* geom, const fpe_scan_params* sp, const fpe_scan* scan) {
    if (!geom) return FPE_E_INVALID_ARG;
    const char* why = nullptr;
    const int rc = fpe::check_map_geometry(geom->rows, geom->cols, geom->resolution, &why);
    if (rc != FPE_OK) return rc;
    return fpe::check_scan(geom->rows, geom->cols, sp, scan, &why);
}

int fpe_scan_clear_params_defaults(fpe_scan_clear_params* out) {
    if (!out) return FPE_E_INVALID_ARG;
    fpe::scan_clear_params_defaults(*out);
    return FPE_OK;
}

int fpe_scan_clear_validate(const fpe_map_desc* geom, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan) {
    if (!geom) return FPE_E_INVALID_ARG;
    const char* why = nullptr;
    const int rc = fpe::check_map_geometry(geom->rows, geom->cols, geom->resolution, &why);
    if (rc != FPE_OK) return rc;
    return fpe::check_scan_clear(geom->rows, geom->cols, sp, cp, scan, &why);
}

int fpe_scan_close_params_defaults(fpe_scan_close_params* out) {
    if (!out) return FPE_E_INVALID_ARG;
    fpe::scan_close_params_defaults(*out);
    return FPE_OK;
}

int fpe_scan_close_validate(const fpe_map_desc* geom, const fpe_scan_close_params* kp, const int32_t rect[4]) {
    if (!geom) return FPE_E_INVALID_ARG;
    const char* why = nullptr;
    const int rc = fpe::check_map_geometry(geom->rows, geom->cols, geom->resolution, &why);
    if (rc != FPE_OK) return rc;
    return fpe::check_scan_close(geom->rows, geom->cols, kp, rect, &why);
}

int fpe_scan_image_validate(const fpe_map_desc* geom, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan,
                            const fpe_scan_image* im) {
    if (!geom) return FPE_E_INVALID_ARG;
    const char* why = nullptr;
    const int rc = fpe::check_map_geometry(geom->rows, geom->cols, geom->resolution, &why);
    if (rc != FPE_OK) return rc;
    return fpe::check_scan_image(geom->rows, geom->cols, sp, cp, scan, im, &why);
}

// The rule of point 6 of the scan block in plain C++: every operation is one f32 operation (this file is built without contraction).
int fpe_scan_image_points(const fpe_scan_image* im, const void* image, float* out_xyz) {
    const char* why = nullptr;
    if (!image || !out_xyz || fpe::check_scan_image_desc(im, &why) != FPE_OK) return FPE_E_INVALID_ARG;
    const int nr = fpe::scan_image_sel_rows(*im), nc = fpe::scan_image_sel_cols(*im);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int ri = 0; ri < nr; ++ri) {
        for (int ci = 0; ci < nc; ++ci) {
            const int v = ri * im->row_step, u = ci * im->col_step;
            const size_t k = static_cast<size_t>(v) * static_cast<size_t>(im->row_pitch) + static_cast<size_t>(u);
            float* o = out_xyz + 3 * (static_cast<size_t>(ri) * nc + ci);
            float d;
            bool valid;
            if (im->format == FPE_SCAN_DEPTH_U16) {
                const uint16_t raw = static_cast<const uint16_t*>(image)[k];
                valid = raw != 0;
                d = static_cast<float>(raw) * im->depth_scale;
            } else {
                const float raw = static_cast<const float*>(image)[k];
                valid = std::isfinite(raw) && raw > 0.0f;
                d = raw * im->depth_scale;
            }
            if (!valid) {
                o[0] = o[1] = o[2] = nan;
            } else if (im->model == FPE_SCAN_IMAGE_PINHOLE) {
                const float xn = (static_cast<float>(u) - im->cx) * d;
                const float yn = (static_cast<float>(v) - im->cy) * d;
                o[0] = xn / im->fx;
                o[1] = yn / im->fy;
                o[2] = d;
            } else {
                const float ce = im->row_dir[2 * v], se = im->row_dir[2 * v + 1];
                const float ca = im->col_dir[2 * u], sa = im->col_dir[2 * u + 1];
                const float w = d * ce;
                o[0] = w * ca;
                o[1] = w * sa;
                o[2] = d * se;
            }
        }
    }
    return FPE_OK;
}

}  // extern "C"

namespace fpe {

void scan_params_defaults(fpe_scan_params& out) {
    out.min_range = 0.1f;
    out.max_range = 10.0f;
    out.min_z = -100.0f;
    out.max_z = 100.0f;
    out.band = 0.05f;
    out.var_base = 1e-4f;
    out.var_range = 1e-4f;
    out.var_min = 1e-6f;
    out.var_max = 1.0f;
    out.gate = 3.0f;
    out.var_outlier = 1e-3f;
    out.replace_count = 0;
}

int check_scan(int rows, int cols, const fpe_scan_params* sp, const fpe_scan* scan, const char** why) {
    auto bad = [&](const char* msg) {
        *why = msg;
        return static_cast<int>(FPE_E_INVALID_ARG);
    };
    if (!sp || !scan) return bad("null scan or scan parameters");
    if (scan->n_points < 0 || scan->n_points > FPE_SCAN_MAX_POINTS) return bad("n_points out of range");
    if (scan->point_stride < 3) return bad("point_stride below 3");
    if (scan->reserved[0] != 0 || scan->reserved[1] != 0) return bad("reserved must be 0");
    const int32_t* roi = scan->roi;
    if (roi[2] <= 0 || roi[3] <= 0) return bad("empty roi");
    if (roi[0] < 0 || roi[1] < 0 || static_cast<int64_t>(roi[0]) + roi[2] > rows || static_cast<int64_t>(roi[1]) + roi[3] > cols)
        return bad("roi outside the state");
    for (double t : scan->sensor_to_map)
        if (!std::isfinite(t)) return bad("non-finite transform");
    const float all[11] = {sp->min_range, sp->max_range, sp->min_z, sp->max_z, sp->band, sp->var_base, sp->var_range, sp->var_min, sp->var_max,
                           sp->gate, sp->var_outlier};
    for (float v : all)
        if (!std::isfinite(v)) return bad("non-finite scan parameter");
    if (sp->min_range > sp->max_range) return bad("min_range above max_range");
    if (sp->min_z > sp->max_z) return bad("min_z above max_z");
    if (std::fabs(sp->min_z) > 16384.0f || std::fabs(sp->max_z) > 16384.0f) return bad("height limits beyond +-16384");
    if (sp->var_base < 0.0f || sp->var_range < 0.0f || sp->var_min < 0.0f || sp->var_max < 0.0f || sp->var_outlier < 0.0f)
        return bad("negative variance parameter");
    if (sp->var_min > sp->var_max) return bad("var_min above var_max");
    if (!(sp->gate > 0.0f)) return bad("gate must be positive");
    if (sp->band < 0.0f) return bad("negative band");
    return FPE_OK;
}

// The constants of a fuse as the kernels take them: every widening and square of the contract formed once, here.
void scan_consts(const fpe_scan_params& sp, const fpe_scan& scan, const MapGeom& g, ScanArgs& a) {
    for (int k = 0; k < 12; ++k) a.T[k] = scan.sensor_to_map[k];
    a.minR2 = static_cast<double>(sp.min_range) * static_cast<double>(sp.min_range);
    a.maxR2 = static_cast<double>(sp.max_range) * static_cast<double>(sp.max_range);
    a.minZ = sp.min_z;
    a.maxZ = sp.max_z;
    a.g = g;
    const double bq = std::rint(static_cast<double>(sp.band) * 65536.0);
    a.bandQ = bq >= 2147483648.0 ? (int64_t{1} << 31) : static_cast<int64_t>(bq);
    a.varBase = sp.var_base;
    a.varRange = sp.var_range;
    a.varMin = sp.var_min;
    a.varMax = sp.var_max;
    a.gate2 = sp.gate * sp.gate;
    a.varOutlier = sp.var_outlier;
    a.replaceCount = sp.replace_count;
    a.n = scan.n_points;
    a.stride = scan.point_stride;
    a.row0 = scan.roi[0];
    a.col0 = scan.roi[1];
    a.nr = scan.roi[2];
    a.nc = scan.roi[3];
    a.im = ScanImage{};  // (the image forms set it)
}

void scan_clear_params_defaults(fpe_scan_clear_params& out) {
    out.sample_step = 0.5f;
    out.margin = 0.10f;
    out.start_samples = 2;
    out.end_samples = 4;
    out.min_hits = 2;
    out.ray_stride = 1;
    out.max_samples = 4096;
    out.reserved = 0;
}

int check_scan_clear(int rows, int cols, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const char** why) {
    const int rc = check_scan(rows, cols, sp, scan, why);
    if (rc != FPE_OK) return rc;
    auto bad = [&](const char* msg) {
        *why = msg;
        return static_cast<int>(FPE_E_INVALID_ARG);
    };
    if (!cp) return bad("null clear parameters");
    if (!std::isfinite(cp->sample_step) || !std::isfinite(cp->margin)) return bad("non-finite clear parameter");
    if (!(cp->sample_step > 0.0f && cp->sample_step <= 1.0f)) return bad("sample_step outside (0, 1]");
    if (cp->margin < 0.0f) return bad("negative margin");
    if (cp->start_samples < 0 || cp->end_samples < 0) return bad("negative start_samples or end_samples");
    if (cp->min_hits < 1) return bad("min_hits below 1");
    if (cp->ray_stride < 1) return bad("ray_stride below 1");
    if (cp->max_samples < 1 || cp->max_samples > 65536) return bad("max_samples outside 1 .. 65536");
    if (cp->reserved != 0) return bad("reserved must be 0");
    return FPE_OK;
}

// The constants of a clear as its kernels take them: the fuse's point tests (scan_consts) and the clear's widenings.
void scan_clear_consts(const fpe_scan_params& sp, const fpe_scan_clear_params& cp, const fpe_scan& scan, const MapGeom& g, ScanClearArgs& a) {
    ScanArgs f;
    scan_consts(sp, scan, g, f);
    for (int k = 0; k < 12; ++k) a.T[k] = f.T[k];
    a.minR2 = f.minR2;
    a.maxR2 = f.maxR2;
    a.minZ = f.minZ;
    a.maxZ = f.maxZ;
    a.g = g;
    a.step = static_cast<double>(cp.sample_step) * g.res;
    a.margin = cp.margin;
    a.maxSamples = cp.max_samples;
    a.startSamples = cp.start_samples;
    a.endSamples = cp.end_samples;
    a.minHits = cp.min_hits;
    a.rayStride = cp.ray_stride;
    a.n = f.n;
    a.stride = f.stride;
    a.nCast = static_cast<int32_t>((static_cast<int64_t>(f.n) + cp.ray_stride - 1) / cp.ray_stride);
    a.row0 = f.row0;
    a.col0 = f.col0;
    a.nr = f.nr;
    a.nc = f.nc;
    a.im = f.im;
}

int check_scan_image_desc(const fpe_scan_image* im, const char** why) {
    auto bad = [&](const char* msg) {
        *why = msg;
        return static_cast<int>(FPE_E_INVALID_ARG);
    };
    if (!im) return bad("null image descriptor");
    if (im->model != FPE_SCAN_IMAGE_PINHOLE && im->model != FPE_SCAN_IMAGE_SPHERICAL) return bad("unknown image model");
    if (im->format != FPE_SCAN_DEPTH_U16 && im->format != FPE_SCAN_DEPTH_F32) return bad("unknown depth format");
    if (im->width < 1 || im->width > 4096 || im->height < 1 || im->height > 4096) return bad("image width or height outside 1 .. 4096");
    if (im->row_pitch < im->width) return bad("row_pitch below width");
    if (im->row_step < 1 || im->col_step < 1) return bad("row_step or col_step below 1");
    if (!std::isfinite(im->depth_scale) || !(im->depth_scale > 0.0f)) return bad("depth_scale must be finite and positive");
    if (im->model == FPE_SCAN_IMAGE_PINHOLE) {
        if (!std::isfinite(im->fx) || !std::isfinite(im->fy) || im->fx == 0.0f || im->fy == 0.0f) return bad("fx and fy must be finite and not 0");
        if (!std::isfinite(im->cx) || !std::isfinite(im->cy)) return bad("cx and cy must be finite");
    } else if (!im->row_dir || !im->col_dir) {
        return bad("a spherical image needs both direction tables");
    }
    if (im->reserved[0] != 0 || im->reserved[1] != 0) return bad("reserved must be 0");
    if (static_cast<int64_t>(scan_image_sel_rows(*im)) * scan_image_sel_cols(*im) > FPE_SCAN_MAX_POINTS) return bad("more selected pixels than FPE_SCAN_MAX_POINTS");
    return FPE_OK;
}

int check_scan_image(int rows, int cols, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const fpe_scan_image* im,
                     const char** why) {
    int rc = cp ? check_scan_clear(rows, cols, sp, cp, scan, why) : check_scan(rows, cols, sp, scan, why);
    if (rc == FPE_OK) rc = check_scan_image_desc(im, why);
    if (rc != FPE_OK) return rc;
    if (scan->n_points != scan_image_sel_rows(*im) * scan_image_sel_cols(*im)) {
        *why = "n_points is not the number of selected pixels";
        return FPE_E_INVALID_ARG;
    }
    return FPE_OK;
}

void scan_image_consts(const fpe_scan_image& im, const void* d_image, const float* d_rowDir, const float* d_colDir, ScanImage& out) {
    out.data = d_image;
    out.rowDir = d_rowDir;
    out.colDir = d_colDir;
    out.model = im.model;
    out.format = im.format;
    out.pitch = im.row_pitch;
    out.rowStep = im.row_step;
    out.colStep = im.col_step;
    out.selCols = scan_image_sel_cols(im);
    out.scale = im.depth_scale;
    out.fx = im.fx;
    out.fy = im.fy;
    out.cx = im.cx;
    out.cy = im.cy;
}

void scan_close_params_defaults(fpe_scan_close_params& out) {
    std::memset(&out, 0, sizeof(out));
    out.reach = 4;
    out.max_gap = 5;
    out.min_axes = 2;
    out.max_spread = 0.08f;
}

int check_scan_close(int rows, int cols, const fpe_scan_close_params* kp, const int32_t rect[4], const char** why) {
    auto bad = [&](const char* msg) {
        *why = msg;
        return static_cast<int>(FPE_E_INVALID_ARG);
    };
    if (!kp || !rect) return bad("null close parameters or rectangle");
    if (kp->reach < 1 || kp->reach > kCloseMaxReach) return bad("reach outside 1 .. 8");
    if (kp->max_gap < 1 || kp->max_gap > 2 * kp->reach - 1) return bad("max_gap outside 1 .. 2 * reach - 1");
    if (kp->min_axes < 1 || kp->min_axes > 4) return bad("min_axes outside 1 .. 4");
    if (!(kp->max_spread >= 0.0f)) return bad("max_spread negative or NaN");
    for (int k = 0; k < 4; ++k)
        if (kp->reserved[k] != 0) return bad("reserved must be 0");
    if (rect[2] < 1 || rect[3] < 1) return bad("empty rectangle");
    if (rect[0] < 0 || rect[1] < 0 || rect[0] > rows - rect[2] || rect[1] > cols - rect[3]) return bad("the rectangle reaches outside the state");
    return FPE_OK;
}

void scan_close_consts(const fpe_scan_close_params& kp, const int32_t rect[4], int rows, int cols, ScanCloseArgs& a) {
    a.rows = rows;
    a.cols = cols;
    a.row0 = rect[0];
    a.col0 = rect[1];
    a.nr = rect[2];
    a.nc = rect[3];
    a.reach = kp.reach;
    a.maxGap = kp.max_gap;
    a.minAxes = kp.min_axes;
    a.maxSpread = kp.max_spread;
    a.outStride = rect[3];
    a.elev = nullptr;
    a.out = nullptr;
    a.cls = nullptr;
    a.acc = nullptr;
    a.info = nullptr;
}

int check_map_update(int rows, int cols, const fpe_map_update* u, bool elevationOnly, const char** why) {
    auto bad = [&](const char* msg) {
        *why = msg;
        return static_cast<int>(FPE_E_INVALID_ARG);
    };
    if (!u) return bad("null map update");
    if (rows <= 0 || cols <= 0) return bad("map size out of range");
    if (u->n_patches < 0 || u->n_patches > FPE_UPDATE_MAX_PATCHES) return bad("n_patches out of range");
    if (u->reserved != 0) return bad("reserved must be 0");
    if (!std::isfinite(u->position[0]) || !std::isfinite(u->position[1])) return bad("bad position");
    for (int k = 0; k < u->n_patches; ++k) {
        const fpe_map_patch& p = u->patch[k];
        if (p.n_rows <= 0 || p.n_cols <= 0) return bad("empty patch rectangle");
        if (p.row0 < 0 || p.col0 < 0 || static_cast<int64_t>(p.row0) + p.n_rows > rows || static_cast<int64_t>(p.col0) + p.n_cols > cols)
            return bad("patch rectangle outside the map");
        if (elevationOnly ? p.traversability != nullptr : !p.traversability) return bad(elevationOnly ? "an elevation update's patches carry no traversability" : "null patch layer");
        if (!p.elevation) return bad("null patch layer");
        const bool rowMajor = p.col_stride == 1 && p.row_stride >= p.n_cols;
        const bool colMajor = p.row_stride == 1 && p.col_stride >= p.n_rows;
        if (!rowMajor && !colMajor) return bad("patch strides are neither row-major nor column-major with a pitch");
    }
    return FPE_OK;
}

int check_map_geometry(int rows, int cols, double res, const char** why) {
    auto bad = [&](const char* msg) {
        *why = msg;
        return static_cast<int>(FPE_E_INVALID_ARG);
    };
    if (rows <= 0 || cols <= 0 || rows > 32768 || cols > 32768) return bad("map size out of range");
    if (!(res > 0.0) || !std::isfinite(res)) return bad("bad resolution");
    return FPE_OK;
}

// ---- the producer's filter chain: what runs, decided on the host (the kernels: fpe_filters.hpp) ---------------------------------
void filter_params_defaults(fpe_filter_params& out) {
    std::memset(&out, 0, sizeof(out));
    out.normal_radius = 0.05;
    out.slope_critical = 1.0;
    out.step_critical = 0.12;
    out.step_first_radius = 0.08;
    out.step_second_radius = 0.08;
    out.step_critical_cells = 4;
    out.roughness_critical = 0.05;
    out.roughness_radius = 0.05;
}

const char* const kBadFilterParams = "filter radii and critical values must be positive and finite";
int filter_consts(const fpe_filter_params& fp, FilterConsts& fc) {
    const double radii[4] = {fp.normal_radius, fp.step_first_radius, fp.step_second_radius, fp.roughness_radius};
    for (double r : radii)
        if (!(r > 0.0) || !std::isfinite(r)) return FPE_E_INVALID_ARG;
    if (!(fp.slope_critical > 0.0) || !(fp.step_critical > 0.0) || !(fp.roughness_critical > 0.0) || fp.step_critical_cells <= 0) return FPE_E_INVALID_ARG;
    fc = FilterConsts{fp.normal_radius, fp.slope_critical, fp.step_critical, fp.step_first_radius, fp.step_second_radius,
                      fp.step_critical_cells, fp.roughness_critical, fp.roughness_radius};
    return FPE_OK;
}

StepShape step_shape(double r, double res, int H, double reach) {
    StepShape sp{};
    for (auto& c : sp.rowW) c = -1;
    sp.ok = 1;
    sp.rowsOk = 1;
    const double r2 = r * r, res2 = res * res;
    // relative margin on squared distances: 1e-7 near the origin; far from it the rounding of the positions themselves
    // (4 ulp of `reach` on a difference of one resolution, twice that on its square), with a factor of 16 to spare.
    // Beyond 1e-3 two neighbouring offsets of a row could both be in doubt: the walking kernels take over.
    const double rel = fmax(1e-7, 16.0 * 8.0 * 2.220446049250313e-16 * reach / res);
    if (rel > 1e-3) {
        sp.ok = sp.rowsOk = 0;
        return sp;
    }
    const double margin = rel * r2;
    for (int o = -H; o <= H; ++o) {
        int w = -1;
        for (int k = 0; k <= H; ++k) {
            const double d2 = (static_cast<double>(o) * o + static_cast<double>(k) * k) * res2;
            if (d2 < r2 - margin) {
                w = k;
            } else if (d2 <= r2 + margin) {  // on the circle: decided per cell
                sp.edgeRows |= 1ull << (o + H);
                for (int sgn = (k == 0 ? 1 : -1); sgn <= 1; sgn += 2) {
                    if (sp.nEdge >= kStepMaxEdge) {
                        sp.ok = 0;  // (the rows' half-widths below stay valid: the normals kernel tests the next column itself)
                    } else {
                        sp.edgeR[sp.nEdge] = static_cast<int8_t>(o);
                        sp.edgeC[sp.nEdge] = static_cast<int8_t>(sgn * k);
                        ++sp.nEdge;
                    }
                }
            }
        }
        sp.rowW[o + H] = static_cast<int8_t>(w);
        if (w >= 0) sp.storeMask |= 1u << w;
        if (w > sp.wMax) sp.wMax = w;
    }
    sp.nClasses = __builtin_popcount(sp.storeMask);
    if (sp.nClasses > kStepMaxClasses) sp.ok = 0;
    return sp;
}

int filter_halo(double r, double res) { return static_cast<int>(r / res) + 1; }

bool filters_supported(const FilterConsts& fc, const MapGeom& g) {
    const double rmax = std::fmax(std::fmax(fc.normalRadius, fc.roughnessRadius), std::fmax(fc.stepFirstRadius, fc.stepSecondRadius));
    return filter_halo(rmax, g.res) <= kFilterMaxH;
}

FilterRoute filter_route(const FilterConsts& fc, const MapGeom& g) {
    FilterRoute rt{};
    rt.hN = filter_halo(fc.normalRadius, g.res);
    rt.hR = filter_halo(fc.roughnessRadius, g.res);
    rt.h1 = filter_halo(fc.stepFirstRadius, g.res);
    rt.h2 = filter_halo(fc.stepSecondRadius, g.res);
    const double reach = std::fmax(std::fabs(g.posX) + g.orgX, std::fabs(g.posY) + g.orgY) + g.res;
    rt.sN = step_shape(fc.normalRadius, g.res, rt.hN, reach);
    rt.s1 = step_shape(fc.stepFirstRadius, g.res, rt.h1, reach);
    rt.s2 = step_shape(fc.stepSecondRadius, g.res, rt.h2, reach);
    // The moment form takes the lattice as EXACT integers; the published filters (and the oracle) sum the cells' rounded f64
    // positions.  Near the origin the two agree far inside a float ulp; at a coordinate of `reach` a position carries an error of
    // ulp(reach) ~ 2e-16 reach against a spacing of res, and the normal follows it: beyond reach / res = 2e5 (2 km at 1 cm, 4e-11
    // relative) the literal walks run instead (at 3 000 km a handful of cells differed by up to 8 float ulps; tests).
    const bool latticeExact = reach / g.res < 2.0e5;
    const bool sameDisc = fc.roughnessRadius == fc.normalRadius;  // the published default chain: both 0.05 m
    if (sameDisc && rt.hN >= 1 && rt.hN <= kMomentMaxH && rt.sN.rowsOk && latticeExact) rt.tF = rt.hN <= kFusedSmallMaxH ? 16 : 32;
    // Tile edge of the row-run launches: 32 (1024 threads) when a tile row with its halo is still one wavefront load and the
    // arrays fit the LDS, else 16.
    // (32 x 16 where a 32-column tile row with its halo is more than one wavefront load or the runs outgrow the LDS: windows of
    // 15-24 cells — 0.08 m at 0.5 cm: against 16 x 16 the runs per cell drop from 3.1 to 2.1 and the CU holds eight wavefronts
    // instead of four)
    // (tile code: 32 = 32 x 32, 24 = 32 rows x 16 columns, 16 = 16 x 16)
    const auto tile_of = [&](int H, int nClasses) {
        if (g.rows < 64 || g.cols < 64) return 16;
        if (32 + 2 * H <= 64 && step_lds_bytes(H, nClasses, 32, 32) <= kFilterMaxLds) return 32;
        if (16 + 2 * H <= 64 && step_lds_bytes(H, nClasses, 32, 16) <= kFilterMaxLds) return 24;
        return 16;
    };
    if (rt.tF) {
        rt.fusedBytes = fused_moment_bytes(rt.hN, kFusedRows, rt.tF);
        const size_t stepBytes = step_lds_bytes(rt.h2, rt.s2.nClasses, kFusedRows, rt.tF);
        if (rt.s2.ok && rt.tF + 2 * rt.h2 <= 64 && stepBytes <= kFilterMaxLds) {
            rt.stepFused = 1;
            if (stepBytes > rt.fusedBytes) rt.fusedBytes = stepBytes;
        }
        if (rt.fusedBytes > kFilterMaxLds) rt.tF = rt.stepFused = 0;
    }
    // The instantiation of each launch.  A row-run window: its tile, and its halo as a compile-time constant (HS) for the windows
    // of the published default chain — 0.08 m at 2 cm and 1 cm (5 and 9 cells; the first window's 32 x 32 form only: the second
    // rides in the fused launch there) and at 0.5 cm (17 cells on 32 x 16); the walking kernel where the shape does not fit the
    // row-run tables or the runs outgrow the LDS.
    const auto window = [&](bool second, int H, const StepShape& sp) {
        const int tcode = tile_of(H, sp.nClasses);
        WindowForm w{};
        w.TR = tcode == 16 ? 16 : 32;
        w.TC = tcode == 32 ? 32 : 16;
        w.ldsBytes = step_lds_bytes(H, sp.nClasses, w.TR, w.TC);
        if (tcode == 32 && !second && (H == 5 || H == 9)) w.HS = H;
        if (tcode == 24 && H == 17) w.HS = H;  // the published windows (0.08 m) at 0.5 cm
        w.kind = sp.ok && w.ldsBytes <= kFilterMaxLds ? WindowForm::kRuns : WindowForm::kWalk;
        if (w.kind == WindowForm::kWalk) w = WindowForm{WindowForm::kWalk, 0, 0, 0, disc_lds_bytes(H)};
        return w;
    };
    rt.first = window(false, rt.h1, rt.s1);
    rt.second = rt.stepFused ? WindowForm{WindowForm::kInFused, 0, 0, 0, 0} : window(true, rt.h2, rt.s2);
    if (rt.tF) {
        // the published default chain at 2 cm and 1 cm (normals 0.05 m, second step window 0.08 m): the step window's halo is a
        // compile-time constant too
        const bool published = rt.stepFused && ((rt.hN == 3 && rt.h2 == 5) || (rt.hN == 6 && rt.h2 == 9));
        rt.fused = FusedForm{rt.hN, rt.tF, published ? rt.h2 : 0};
    }
    rt.travOnly = rt.tF != 0 && rt.stepFused != 0;
    rt.regionOk = rt.travOnly && rt.first.kind == WindowForm::kRuns;
    return rt;
}

// How far, in cells (Chebyshev), a changed elevation cell can reach into the traversability layer: the widest of the normals'
// and the roughness disc and the two step windows one behind the other (a step value reads step heights within h2, each of which
// reads elevations within h1).
int filter_reach_cells(const FilterConsts& fc, double res) {
    const int hN = filter_halo(fc.normalRadius, res), hR = filter_halo(fc.roughnessRadius, res);
    const int h1 = filter_halo(fc.stepFirstRadius, res), h2 = filter_halo(fc.stepSecondRadius, res);
    return std::max(std::max(hN, hR), h1 + h2);
}

// ---- region launches of the traversability-only chain (fpe_update_elevation*) ---------------------------------------------------
// Cells of the union of a few rectangles: coordinate compression (at most 2 n cuts per axis).
int64_t cell_rects_union(const CellRect* r, int n, int rows, int cols) {
    std::vector<int> ys(2 * static_cast<size_t>(n)), xs(2 * static_cast<size_t>(n));
    int ny = 0, nx = 0;
    const auto clip = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
    for (int k = 0; k < n; ++k) {
        ys[ny++] = clip(r[k].r0, rows);
        ys[ny++] = clip(r[k].r1, rows);
        xs[nx++] = clip(r[k].c0, cols);
        xs[nx++] = clip(r[k].c1, cols);
    }
    std::sort(ys.begin(), ys.end());
    std::sort(xs.begin(), xs.end());
    int64_t cells = 0;
    for (int a = 0; a + 1 < ny; ++a)
        for (int b = 0; b + 1 < nx; ++b) {
            if (ys[a] == ys[a + 1] || xs[b] == xs[b + 1]) continue;
            for (int k = 0; k < n; ++k)
                if (r[k].r0 <= ys[a] && ys[a + 1] <= r[k].r1 && r[k].c0 <= xs[b] && xs[b + 1] <= r[k].c1) {
                    cells += static_cast<int64_t>(ys[a + 1] - ys[a]) * (xs[b + 1] - xs[b]);
                    break;
                }
        }
    return cells;
}
bool filters_region_plan(const MapGeom& g, const FilterRoute& rt, const CellRect* dirty, int nDirty, FilterRegion* out) {
    if (nDirty < 0 || nDirty > kRegionMaxRects || !rt.regionOk) return false;
    const int TR1 = rt.first.TR, TC1 = rt.first.TC, TRf = kFusedRows, TCf = rt.fused.TC;
    FilterRegion rg{};
    CellRect cover[kRegionMaxRects];
    for (int k = 0; k < nDirty; ++k) {
        const CellRect& d = dirty[k];
        if (d.r0 < 0 || d.c0 < 0 || d.r1 > g.rows || d.c1 > g.cols || d.r0 >= d.r1 || d.c0 >= d.c1) return false;
        const int ty0 = d.r0 / TRf, ty1 = (d.r1 - 1) / TRf + 1, tx0 = d.c0 / TCf, tx1 = (d.c1 - 1) / TCf + 1;
        rg.fused.r[k] = TileRect{ty0, tx0, ty1 - ty0, tx1 - tx0};
        rg.fused.nBlocks += (ty1 - ty0) * (tx1 - tx0);
        cover[k] = CellRect{ty0 * TRf, tx0 * TCf, std::min(ty1 * TRf, g.rows), std::min(tx1 * TCf, g.cols)};
        // the step heights those tiles read: their cells grown by the second window's halo, clipped to the map
        const int r0 = std::max(cover[k].r0 - rt.h2, 0), r1 = std::min(cover[k].r1 + rt.h2, g.rows);
        const int c0 = std::max(cover[k].c0 - rt.h2, 0), c1 = std::min(cover[k].c1 + rt.h2, g.cols);
        const int sy0 = r0 / TR1, sy1 = (r1 - 1) / TR1 + 1, sx0 = c0 / TC1, sx1 = (c1 - 1) / TC1 + 1;
        rg.step.r[k] = TileRect{sy0, sx0, sy1 - sy0, sx1 - sx0};
        rg.step.nBlocks += (sy1 - sy0) * (sx1 - sx0);
    }
    rg.fused.n = rg.step.n = nDirty;
    rg.recomputed = cell_rects_union(cover, nDirty, g.rows, g.cols);
    *out = rg;
    return true;
}

// The dirty set D of include/fpe.h as rectangles: the patch rectangles and the bands without a source grown by R, and the bands
// whose window the map edge clips differently before and after the move — whole rows / columns, found as runs of per-line flags.
void elevation_dirty_rects(int rows, int cols, int R, int sr, int sc, const fpe_map_update* u, std::vector<CellRect>& out) {
    out.clear();
    if (std::abs(sr) >= rows || std::abs(sc) >= cols) {  // nothing is carried: every cell is without a source
        out.push_back(CellRect{0, 0, rows, cols});
        return;
    }
    const auto line_runs = [&](int n, int s, bool rowAxis) {
        std::vector<uint8_t> flag(static_cast<size_t>(n), 0);
        for (int i = 0; i < n; ++i) {
            // C grown by R: some line within R has no source
            const int lo = std::max(i - R, 0), hi = std::min(i + R, n - 1);
            const bool noSource = s > 0 ? hi + s >= n : (s < 0 ? lo + s < 0 : false);
            const bool clipped = s != 0 && (i < R || i >= n - R || i + s < R || i + s >= n - R);  // B
            flag[static_cast<size_t>(i)] = noSource || clipped;
        }
        for (int i = 0; i < n;) {
            if (!flag[static_cast<size_t>(i)]) {
                ++i;
                continue;
            }
            int j = i;
            while (j < n && flag[static_cast<size_t>(j)]) ++j;
            out.push_back(rowAxis ? CellRect{i, 0, j, cols} : CellRect{0, i, rows, j});
            i = j;
        }
    };
    line_runs(rows, sr, true);
    line_runs(cols, sc, false);
    for (int k = 0; k < u->n_patches; ++k) {
        const fpe_map_patch& p = u->patch[k];
        const CellRect r{std::max(p.row0 - R, 0), std::max(p.col0 - R, 0), static_cast<int32_t>(std::min<int64_t>(static_cast<int64_t>(p.row0) + p.n_rows + R, rows)),
                         static_cast<int32_t>(std::min<int64_t>(static_cast<int64_t>(p.col0) + p.n_cols + R, cols))};
        bool inside = false;  // (a rectangle inside an earlier one adds nothing)
        for (const CellRect& q : out) inside = inside || (q.r0 <= r.r0 && r.r1 <= q.r1 && q.c0 <= r.c0 && r.c1 <= q.c1);
        if (!inside) out.push_back(r);
    }
}

int plan_elevation_update(int rows, int cols, double res, const fpe_filter_params* fp, const fpe_map_update* u, ElevationUpdatePlan& plan, const char** why) {
    auto bad = [&](int rc, const char* msg) {
        *why = msg;
        return rc;
    };
    int rc = check_map_update(rows, cols, u, true, why);
    if (rc != FPE_OK) return rc;
    rc = check_map_geometry(rows, cols, res, why);
    if (rc != FPE_OK) return rc;
    fpe_filter_params def;
    if (!fp) {
        filter_params_defaults(def);
        fp = &def;
    }
    if (filter_consts(*fp, plan.fc) != FPE_OK) return bad(FPE_E_INVALID_ARG, kBadFilterParams);
    plan.g = make_geom(rows, cols, res, u->position[0], u->position[1]);
    if (!filters_supported(plan.fc, plan.g)) return bad(FPE_E_UNSUPPORTED, "filter radius spans more cells than the stencil tables hold");
    plan.rt = filter_route(plan.fc, plan.g);
    plan.sr = std::max(-rows, std::min(rows, u->shift[0]));  // beyond +-rows nothing is carried either way
    plan.sc = std::max(-cols, std::min(cols, u->shift[1]));
    const int R = filter_reach_cells(plan.fc, res);
    elevation_dirty_rects(rows, cols, R, plan.sr, plan.sc, u, plan.dirty);
    plan.info.reach_cells = R;
    plan.info.dirty_cells = cell_rects_union(plan.dirty.data(), static_cast<int>(plan.dirty.size()), rows, cols);
    const bool carried = std::abs(plan.sr) < rows && std::abs(plan.sc) < cols;
    const bool region = carried && static_cast<int>(plan.dirty.size()) <= kRegionMaxRects &&
                        filters_region_plan(plan.g, plan.rt, plan.dirty.data(), static_cast<int>(plan.dirty.size()), &plan.region);
    plan.info.route = region ? 0 : 1;
    plan.info.recomputed_cells = region ? plan.region.recomputed : static_cast<int64_t>(rows) * cols;
    return FPE_OK;
}

}  // namespace fpe
