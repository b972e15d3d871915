// fpe_trunk.hpp — part twelve of the kernel translation unit (included last in fpe_kernels.hip, behind fpe_swing.hpp, inside namespace
// fpe): trunk checks (fpe_trunk_*, include/fpe.h) — the body box of each stance of a plan, or of an arbitrary stance, against the
// elevation layer.  The totalOrder keys and the width-16 reductions are fpe_swing.hpp's.
//
//   trunk_stances_kernel<kPlan>   ONE body for both forms.  Sixteen lanes per stance, four stances per wavefront, sixteen per
//                          workgroup; no LDS, no atomics, no scratch.  kPlan = false: stance s is query s.  kPlan = true: stance
//                          s = b * nCycles + g is formed here from the plan's nominal records of cycle g (four 32-byte records, read by
//                          all sixteen lanes at one address) and cycle_ok[s].
//                          The sixteen lanes are the COLUMNS of a box row: the canonical layer is row-major, so the members of a row are
//                          consecutive floats (the yaml body of 0.4387 x 0.175 m is about 23 x 9, 45 x 18 and 89 x 36 cells at 2, 1 and
//                          0.5 cm).  A box wider than sixteen columns is taken in groups of sixteen columns.  The members are an exact
//                          index rectangle: a COLUMN's membership (fabs(py - cy) <= hy) and its term slope_y * (py - cy) are computed
//                          once, when the lane takes the column; a ROW's membership and slope_x * (px - cx) once per row of a column
//                          group (the sixteen lanes of a group compute the same row values: that is one instruction each, not
//                          sixteen).  A member cell then costs its load, the known test, the contract's two adds and one subtract, and
//                          a key compare — no division, no multiplication by a cell.  The enumerated rectangle only has to be a
//                          SUPERSET of the members (proof at trunk_box); the contract's two fabs tests decide.
//                          A lane meets the rows of its column in ascending order, so `>` alone keeps the lowest row of equal gaps
//                          within a column; columns and lanes are merged under (gap ascending, cell index ascending), the cell index
//                          i * cols + j ordering as (row, column).  The minimum is kept as the maximum of the complemented key, so
//                          the reductions of the swing check serve.  Lane 0 stores the 56-byte record.
//   trunk_summary_kernel   sixteen lanes per pose over its nCycles records: extrema, counts and the first bad cycle, combined the same
//                          way.  No atomics: every byte is a function of the inputs alone.
#pragma once

namespace {

// What px - cx (and py - cy) as computed can differ by from the real difference of the real cell centre and the real box centre, in
// metres, for |foot coordinate| <= 1e6 and |cell coordinate| <= 2e6 (swing_map_supported): res * double(-i), base + (..), the three
// sums and the product behind cx, and the difference itself each round to half an ulp of at most 4e6, 2^-32 m — seven such steps stay
// below 1.7e-9.  The enumeration allows 1e-8, as the swing check does.
constexpr double kTrunkEta = kSwingEta;

// A stance as the kernel body takes it
struct TrunkStance {
    double x[4], y[4], z[4];  // RF, RH, LH, LF
    float halfLength, halfWidth;  // as given: <= 0 means the call's default
};

// The index rectangle the lanes look at.  CLAIM: every member (i, j) has iLo <= i <= iHi and jLo <= j <= jHi as computed below (before
// the clamps to the map, which only drop cells that are no cells).
// PROOF, for the rows (the columns alike).  Let i be the row of a member: the contract found fabs(fl(px - cx)) <= hx, so the real
// centre X_i = baseX - res * i satisfies |X_i - cx| <= hx + kTrunkEta =: rho (see kTrunkEta), that is
//     (baseX - (cx + rho)) / res  <=  i  <=  (baseX - (cx - rho)) / res          in real arithmetic.
// The code computes both quotients as fl(fl(baseX - fl(cx +- rho)) * rinv) with rinv = fl(1 / res): two roundings of at most 2^-32 m
// in the numerator (2^-32 / res <= 2.4e-6 cells for res >= 1e-4) and a relative error below 3.4e-16 on a quotient of at most
// 4e6 / 1e-4 = 4e10 cells (1.4e-5 cells): qLo' and qHi' are each within eps < 1e-4 of the real bounds.  i is an integer with
// i >= qLo' - eps > floor(qLo') - 1, so i >= floor(qLo'); and i <= qHi' + eps < floor(qHi') + 1 + eps, so i <= floor(qHi') + 1.
struct TrunkBox {
    int iLo, iHi, jLo, jHi;  // clamped to the map; lo > hi: nothing
};
FPE_HD TrunkBox trunk_box(const MapGeom& g, double cx, double cy, double hx, double hy) {
    const double rx = hx + kTrunkEta, ry = hy + kTrunkEta;
    TrunkBox w;
    w.iLo = swing_clamp_index(0.0, floor((g.baseX - (cx + rx)) * g.rinv), static_cast<double>(g.rows));
    w.iHi = swing_clamp_index(-1.0, floor((g.baseX - (cx - rx)) * g.rinv) + 1.0, static_cast<double>(g.rows - 1));
    w.jLo = swing_clamp_index(0.0, floor((g.baseY - (cy + ry)) * g.rinv), static_cast<double>(g.cols));
    w.jHi = swing_clamp_index(-1.0, floor((g.baseY - (cy - ry)) * g.rinv) + 1.0, static_cast<double>(g.cols - 1));
    return w;
}

// The cell cap of include/fpe.h, on the host and on the device alike
FPE_HD bool trunk_box_over_cap(double hx, double hy, double res) {
    return (2.0 * hx / res + 3.0) * (2.0 * hy / res + 3.0) > static_cast<double>(FPE_TRUNK_MAX_CELLS);
}

// What the contract derives from a stance ahead of any cell
struct TrunkFrame {
    double cx, cy, hx, hy, slopeX, slopeY, baseZ;
    bool degenerate;
};
// Fills `t` and returns whether the stance is one the host forms refuse (and the device forms answer with FPE_TRUNK_REFUSED): a
// non-finite or over-bound coordinate or half extent, a box over the cell cap, a slope beyond the bound.  One function for the
// kernel and for the host forms' check (trunk_stance_refused), so that both decide by the same expressions.
FPE_HD bool trunk_frame(const TrunkConsts& tc, const TrunkStance& s, double res, TrunkFrame& t) {
    bool bad = !(fabs(static_cast<double>(s.halfLength)) <= DBL_MAX) || !(fabs(static_cast<double>(s.halfWidth)) <= DBL_MAX);  // not finite
    for (int k = 0; k < 4; ++k) bad = bad || !(fabs(s.x[k]) <= 1e6) || !(fabs(s.y[k]) <= 1e6) || !(fabs(s.z[k]) <= 1e6);  // (NaN fails)
    t.hx = s.halfLength > 0.0f ? static_cast<double>(s.halfLength) : tc.defaultHx;
    t.hy = s.halfWidth > 0.0f ? static_cast<double>(s.halfWidth) : tc.defaultHy;
    bad = bad || t.hx > static_cast<double>(FPE_TRUNK_MAX_HALF_EXTENT) || t.hy > static_cast<double>(FPE_TRUNK_MAX_HALF_EXTENT);
    bad = bad || trunk_box_over_cap(t.hx, t.hy, res);
    t.cx = ((s.x[0] + s.x[1]) + (s.x[2] + s.x[3])) * 0.25;
    t.cy = ((s.y[0] + s.y[1]) + (s.y[2] + s.y[3])) * 0.25;
    const double zm = ((s.z[0] + s.z[1]) + (s.z[2] + s.z[3])) * 0.25;
    const double dxf = ((s.x[0] + s.x[3]) - (s.x[1] + s.x[2])) * 0.5, dzf = ((s.z[0] + s.z[3]) - (s.z[1] + s.z[2])) * 0.5;
    const double dyl = ((s.y[2] + s.y[3]) - (s.y[0] + s.y[1])) * 0.5, dzl = ((s.z[2] + s.z[3]) - (s.z[0] + s.z[1])) * 0.5;
    t.slopeX = dxf > 0.0 ? dzf / dxf : 0.0;
    t.slopeY = dyl > 0.0 ? dzl / dyl : 0.0;
    t.baseZ = zm + tc.rideHeight;
    t.degenerate = !(dxf > 0.0) || !(dyl > 0.0);
    return bad || !(fabs(t.slopeX) <= FPE_TRUNK_MAX_SLOPE) || !(fabs(t.slopeY) <= FPE_TRUNK_MAX_SLOPE);
}

// The record of one stance, computed by the sixteen lanes of its group (all of them active); every lane returns it.
__device__ __forceinline__ fpe_trunk_record trunk_stance_record(const DevMap& m, const TrunkConsts& tc, const TrunkStance& s, int lane) {
    fpe_trunk_record rec{};
    const MapGeom& g = m.g;
    TrunkFrame t;
    if (trunk_frame(tc, s, g.res, t)) {
        rec.flags = FPE_TRUNK_REFUSED;
        return rec;
    }
    const double cx = t.cx, cy = t.cy, hx = t.hx, hy = t.hy, slopeX = t.slopeX, slopeY = t.slopeY, baseZ = t.baseZ;
    const bool offMap = !(within_axis(cx + hx, g.orgX, g.posX, g.lenX) && within_axis(cx - hx, g.orgX, g.posX, g.lenX) &&
                          within_axis(cy + hy, g.orgY, g.posY, g.lenY) && within_axis(cy - hy, g.orgY, g.posY, g.lenY));
    const TrunkBox w = trunk_box(g, cx, cy, hx, hy);
    long long bestKey = kSwingNoKey64;  // the complement of the lowest gap's key: no known member yet
    int bestCell = 0x7FFFFFFF;          // i * cols + j (below 2^30: check_map_geometry), so the lowest (row, column) is the lowest value
    int elevKey = kSwingNoKey32;
    int nCells = 0, nUnknown = 0;
    for (int j0 = w.jLo; j0 <= w.jHi; j0 += kSwingLanes) {
        const int j = j0 + lane;
        const double ddy = cell_pos(g.baseY, g.res, j) - cy;
        const bool colIn = j <= w.jHi && fabs(ddy) <= hy;
        const double sy = slopeY * ddy;
        long long colKey = kSwingNoKey64;
        int colCell = 0x7FFFFFFF;
        for (int i = w.iLo; i <= w.iHi; ++i) {
            const double ddx = cell_pos(g.baseX, g.res, i) - cx;
            if (fabs(ddx) <= hx && colIn) {
                const int cell = i * g.cols + j;
                const float e = m.elev[cell];
                ++nCells;
                if (isfinite(e) && e < 10.0f) {
                    const long long key = ~swing_key64((baseZ + (slopeX * ddx + sy)) - static_cast<double>(e));
                    if (key > colKey) {
                        colKey = key;
                        colCell = cell;
                    }
                    elevKey = max(elevKey, swing_key32(e));
                } else {
                    ++nUnknown;
                }
            }
        }
        if (colKey > bestKey || (colKey == bestKey && colCell < bestCell)) {
            bestKey = colKey;
            bestCell = colCell;
        }
    }
    // across the sixteen lanes: the lowest gap, then the lowest cell among the lanes that hold it
    const long long topKey = swing_max64(bestKey);
    const int cell = swing_min32(bestKey == topKey ? bestCell : 0x7FFFFFFF);
    elevKey = swing_max32(elevKey);
    nCells = swing_sum32(nCells);
    nUnknown = swing_sum32(nUnknown);
    const bool known = topKey != kSwingNoKey64;
    rec.clearance = known ? swing_unkey64(~topKey) : __longlong_as_double(0x7FF0000000000000ll);
    rec.slope_x = slopeX;
    rec.slope_y = slopeY;
    rec.base_z = baseZ;
    rec.max_elevation = known ? swing_unkey32(elevKey) : 0.0f;
    rec.n_cells = nCells;
    rec.n_unknown = nUnknown;
    rec.row = known ? cell / g.cols : -1;
    rec.col = known ? cell % g.cols : -1;
    rec.flags = static_cast<uint8_t>(FPE_TRUNK_STANCE | (offMap ? FPE_TRUNK_OFF_MAP : 0u) | (nCells == 0 ? FPE_TRUNK_EMPTY : 0u) |
                                     (nUnknown > 0 ? FPE_TRUNK_UNKNOWN : 0u) |
                                     (rec.clearance < tc.minClearance ? FPE_TRUNK_UNDER_CLEARANCE : 0u) |
                                     ((fabs(slopeX) > tc.maxSlopeX || fabs(slopeY) > tc.maxSlopeY) ? FPE_TRUNK_OVER_SLOPE : 0u) |
                                     (t.degenerate ? FPE_TRUNK_DEGENERATE : 0u));
    return rec;
}

// kPlan false: q[n] -> out[n].  kPlan true: n = B * nCycles stances from nominal and cycleOk.
// Full occupancy: eight wavefronts per SIMD.
template <bool kPlan>
__global__ __launch_bounds__(256, 8) void trunk_stances_kernel(DevMap m, TrunkConsts tc, const fpe_trunk_query* __restrict__ q,
                                                               const fpe_foothold* __restrict__ nominal,
                                                               const uint8_t* __restrict__ cycleOk, int nCycles, int n,
                                                               fpe_trunk_record* __restrict__ out) {
    const int st = static_cast<int>(blockIdx.x) * kSwingPerBlock + static_cast<int>(threadIdx.x) / kSwingLanes;
    const int lane = static_cast<int>(threadIdx.x) & (kSwingLanes - 1);
    if (st >= n) return;  // (a whole group of sixteen lanes at a time: the shuffles stay inside a group)
    TrunkStance s;
    fpe_trunk_record rec{};
    if constexpr (kPlan) {
        if (cycleOk[st] != 0) {
#pragma unroll
            for (int leg = 0; leg < 4; ++leg) {
                const fpe_foothold f = nominal[static_cast<size_t>(st) * 4 + leg];
                s.x[leg] = f.x, s.y[leg] = f.y, s.z[leg] = static_cast<double>(f.z);
            }
            s.halfLength = s.halfWidth = 0.0f;
            rec = trunk_stance_record(m, tc, s, lane);
        }
        rec.gait_cycle_id = static_cast<uint8_t>(st % nCycles);
    } else {
        const fpe_trunk_query& qq = q[st];
#pragma unroll
        for (int leg = 0; leg < 4; ++leg) s.x[leg] = qq.feet[leg][0], s.y[leg] = qq.feet[leg][1], s.z[leg] = qq.feet[leg][2];
        s.halfLength = qq.half_length;
        s.halfWidth = qq.half_width;
        rec = trunk_stance_record(m, tc, s, lane);
    }
    if (lane == 0) out[st] = rec;
}

// Sixteen lanes per pose over its nCycles records (include/fpe.h: fpe_trunk_summary)
__global__ __launch_bounds__(256, 8) void trunk_summary_kernel(const fpe_trunk_record* __restrict__ records, int B, int nCycles,
                                                               fpe_trunk_summary* __restrict__ summary) {
    const int b = static_cast<int>(blockIdx.x) * kSwingPerBlock + static_cast<int>(threadIdx.x) / kSwingLanes;
    const int lane = static_cast<int>(threadIdx.x) & (kSwingLanes - 1);
    if (b >= B) return;
    const fpe_trunk_record* __restrict__ rec = records + static_cast<size_t>(b) * nCycles;
    constexpr uint32_t kBad = FPE_TRUNK_UNDER_CLEARANCE | FPE_TRUNK_OVER_SLOPE;
    constexpr uint32_t kUnknown = FPE_TRUNK_UNKNOWN | FPE_TRUNK_EMPTY | FPE_TRUNK_OFF_MAP;
    long long clearKey = kSwingNoKey64;  // the complement of the lowest clearance's key
    long long sxKey = 0, syKey = 0;      // fabs(slope) is >= +0.0: its bit patterns order as integers
    int nStances = 0, nBad = 0, nUnknown = 0, firstBad = 255;
    for (int k = lane; k < nCycles; k += kSwingLanes) {
        const uint32_t f = rec[k].flags;
        if (!(f & FPE_TRUNK_STANCE)) continue;
        ++nStances;
        clearKey = max(clearKey, ~swing_key64(rec[k].clearance));
        sxKey = max(sxKey, __double_as_longlong(fabs(rec[k].slope_x)));
        syKey = max(syKey, __double_as_longlong(fabs(rec[k].slope_y)));
        if (f & kBad) {
            ++nBad;
            firstBad = min(firstBad, k);
        }
        if (f & kUnknown) ++nUnknown;
    }
    clearKey = swing_max64(clearKey);
    sxKey = swing_max64(sxKey);
    syKey = swing_max64(syKey);
    nStances = swing_sum32(nStances);
    nBad = swing_sum32(nBad);
    nUnknown = swing_sum32(nUnknown);
    firstBad = swing_min32(firstBad);
    if (lane != 0) return;
    fpe_trunk_summary s{};
    s.min_clearance = nStances > 0 ? swing_unkey64(~clearKey) : __longlong_as_double(0x7FF0000000000000ll);
    s.max_abs_slope_x = __longlong_as_double(sxKey);
    s.max_abs_slope_y = __longlong_as_double(syKey);
    s.n_stances = nStances;
    s.n_bad = nBad;
    s.n_unknown = nUnknown;
    s.first_bad_cycle = static_cast<uint8_t>(firstBad);
    summary[b] = s;
}

}  // namespace

bool trunk_box_supported(double hx, double hy, double res) { return !trunk_box_over_cap(hx, hy, res); }

bool trunk_stance_refused(const TrunkConsts& tc, const fpe_trunk_query& q, double res) {
    TrunkStance s;
    for (int leg = 0; leg < 4; ++leg) s.x[leg] = q.feet[leg][0], s.y[leg] = q.feet[leg][1], s.z[leg] = q.feet[leg][2];
    s.halfLength = q.half_length;
    s.halfWidth = q.half_width;
    TrunkFrame t;
    return trunk_frame(tc, s, res, t);
}

hipError_t launch_trunk_stances(const DevMap& m, const TrunkConsts& tc, const fpe_trunk_query* d_q, int n, fpe_trunk_record* d_out,
                                hipStream_t stream) {
    hipLaunchKernelGGL(trunk_stances_kernel<false>, dim3((n + kSwingPerBlock - 1) / kSwingPerBlock), dim3(256), 0, stream, m, tc, d_q,
                       static_cast<const fpe_foothold*>(nullptr), static_cast<const uint8_t*>(nullptr), 0, n, d_out);
    return hipGetLastError();
}

// d_records: B * nCycles records (required: the summary reads them); d_summary: B elements, or null
hipError_t launch_trunk_plan(const DevMap& m, const TrunkConsts& tc, const fpe_foothold* d_nominal, const uint8_t* d_cycleOk, int B,
                             int nCycles, fpe_trunk_record* d_records, fpe_trunk_summary* d_summary, hipStream_t stream) {
    const int n = B * nCycles;
    hipLaunchKernelGGL(trunk_stances_kernel<true>, dim3((n + kSwingPerBlock - 1) / kSwingPerBlock), dim3(256), 0, stream, m, tc,
                       static_cast<const fpe_trunk_query*>(nullptr), d_nominal, d_cycleOk, nCycles, n, d_records);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !d_summary) return e;
    hipLaunchKernelGGL(trunk_summary_kernel, dim3((B + kSwingPerBlock - 1) / kSwingPerBlock), dim3(256), 0, stream, d_records, B, nCycles,
                       d_summary);
    return hipGetLastError();
}
