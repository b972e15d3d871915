// fpe_swing.hpp — part eleven of the kernel translation unit (included at the end of fpe_kernels.hip, inside namespace fpe):
// swing checks (fpe_swing_*, include/fpe.h) — each step of a plan, or an arbitrary segment, against the elevation layer.
//
//   swing_segments_kernel<kPlan>   ONE body for both forms.  Sixteen lanes per segment, four segments per wavefront, sixteen per
//                          workgroup; no LDS, no atomics, no scratch.  kPlan = false: segment s is query s.  kPlan = true: segment
//                          s = (b * nCycles + g) * 4 + leg is formed here from the plan's products, so the four segments of a
//                          wavefront quarter are the four legs of one (b, g): they share the cycle_ok bytes they read and their
//                          capsules lie within a body length of each other in the map.
//                          The sixteen lanes are the COLUMNS of a box row: the canonical layer is row-major, so the members of a row
//                          are consecutive floats (a forward step of foot radius 0.02 m spans 3 to 9 columns at 2 to 0.5 cm), and an
//                          inner loop takes wider rows in groups of sixteen.  The lanes walk the rows of the capsule's x extent; per
//                          row the column interval comes from the part of the segment within reach of that row (swing_row_columns),
//                          so the work follows the capsule's area, not the bounding box of a diagonal.  Every enumerated cell is
//                          decided by the contract's membership expression; the enumeration only has to be a SUPERSET of the members
//                          (proof at swing_row_columns).  A lane keeps its best cell under (lift descending, row, column ascending)
//                          — it meets its cells in ascending (row, column) order, so `>` alone does that — and the sixteen lanes
//                          combine with xor shuffles of width 16 (one DPP row): the maximum lift key, the lowest cell among the
//                          lanes that hold it, the maximum elevation key, the two counts.  Lane 0 stores the 48-byte record.
//   swing_summary_kernel   sixteen lanes per pose over its nCycles * 4 records: maxima, counts and the first cycle with an OVER bit,
//                          combined the same way.  No atomics: every byte is a function of the inputs alone.
#pragma once

namespace {

constexpr int kSwingLanes = 16;           // lanes per segment (and per pose of the summary)
constexpr int kSwingPerBlock = 256 / kSwingLanes;
// What the f64 expressions of the membership test can be off by, in metres, for |segment coordinate| <= 1e6 and |cell coordinate| <=
// 2e6 (swing_map_supported): each of px - ax, t * dx, ax + t * dx, px - (..) rounds to half an ulp of at most 4e6, 2^-31 m — five such
// steps stay below 2.4e-9.  The enumeration allows 1e-8.
constexpr double kSwingEta = 1e-8;
constexpr long long kSwingNoKey64 = -0x7FFFFFFFFFFFFFFFll - 1;  // below the key of every finite value
constexpr int kSwingNoKey32 = -0x7FFFFFFF - 1;

// IEEE-754 totalOrder as a signed integer order (finite values and infinities; a NaN never gets here)
__device__ __forceinline__ long long swing_key64(double v) {
    const long long b = __double_as_longlong(v);
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFll);
}
__device__ __forceinline__ double swing_unkey64(long long k) { return __longlong_as_double(k ^ ((k >> 63) & 0x7FFFFFFFFFFFFFFFll)); }
__device__ __forceinline__ int swing_key32(float v) {
    const int b = __float_as_int(v);
    return b ^ ((b >> 31) & 0x7FFFFFFF);
}
__device__ __forceinline__ float swing_unkey32(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7FFFFFFF)); }

__device__ __forceinline__ long long swing_max64(long long v) {
#pragma unroll
    for (int o = kSwingLanes / 2; o > 0; o >>= 1) {
        const long long w = __shfl_xor(v, o, kSwingLanes);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long swing_min64u(unsigned long long v) {
#pragma unroll
    for (int o = kSwingLanes / 2; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, kSwingLanes);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ int swing_max32(int v) {
#pragma unroll
    for (int o = kSwingLanes / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kSwingLanes));
    return v;
}
__device__ __forceinline__ int swing_min32(int v) {
#pragma unroll
    for (int o = kSwingLanes / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, kSwingLanes));
    return v;
}
__device__ __forceinline__ int swing_sum32(int v) {
#pragma unroll
    for (int o = kSwingLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kSwingLanes);
    return v;
}

// A segment as the kernel body takes it
struct SwingSeg {
    double ax, ay, az, bx, by, bz;
    float radius;  // as given: <= 0 means the call's default
};

// What the host forms refuse, decided per segment on the device: a non-finite coordinate or radius, |coordinate| > 1e6, a radius
// above FPE_SWING_MAX_RADIUS.  r: the resolved radius.
__device__ __forceinline__ bool swing_refused(const SwingSeg& s, float defaultRadius, float& r) {
    const double c[6] = {s.ax, s.ay, s.az, s.bx, s.by, s.bz};
    bool bad = !isfinite(s.radius);
#pragma unroll
    for (int k = 0; k < 6; ++k) bad = bad || !(fabs(c[k]) <= 1e6);  // (NaN and infinities fail the comparison)
    r = s.radius > 0.0f ? s.radius : defaultRadius;
    return bad || r > FPE_SWING_MAX_RADIUS;
}

// The rows and, per row, the columns the lanes look at.  CLAIM: every member (i, j) of the capsule lies in rows [iLo, iHi] and, in its
// row, in columns [jLo, jHi] as computed below (before the clamps to the map, which only drop cells that are no cells).
// PROOF.  Let (i, j) be a member, P = (px, py) its centre as cell_pos returns it, and t^ the (clamped, hence in [0, 1]) parameter the
// membership expression computed for it.  The expression found fl(ex^2 + ey^2) <= fl(r^2), so |ex|, |ey| <= r (1 + 2^-51) as computed;
// with S(t) = A + t (B - A) in real arithmetic, the computed ex differs from px - Sx(t^) by less than kSwingEta (see there), ey alike.
// Hence, with rho = r + kSwingEta (r <= 0.5 absorbs the relative term):   |px - Sx(t^)| <= rho   and   |py - Sy(t^)| <= rho.   (*)
//  Rows.  Sx(t^) lies between ax and bx, so px is in [min(ax, bx) - rho, max(ax, bx) + rho].  px = baseX - res * i up to 2^-31 m, so
//   i lies between the real quotients (baseX - (xmax + rho)) / res and (baseX - (xmin - rho)) / res up to 2^-31 / res.  The computed
//   quotients (n * fl(1 / res): relative error 3.4e-16 of at most 4e6 / res) are off by far less than one for res >= 1e-4
//   (swing_map_supported), so floor(lower) - 1 <= i <= floor(upper) + 2.
//  Columns of row i.  By (*) t^ is in T = {t in [0, 1] : |ax + t dx - px| <= rho}, an interval.  When |dx| <= max(2 rho, res) the
//   code takes [0, 1], a superset of T.  Otherwise T is [tm - hw, tm + hw] cut to [0, 1] with tm = (px - ax) / dx and hw = rho / |dx|
//   < 1/2, so |tm| < 3/2 in a row that has a member; the code computes both with fl(1 / dx) and is off by at most 2.4e-9 / |dx| + 1e-15
//   there.  Sy is linear, so Sy(t^) lies between Sy at the ends of T, and the computed ends y0, y1 are off by at most
//   |dy| (2.4e-9 / |dx| + 1e-15) + 2^-31 <= kSwingEta (1 + |dy| / |dx|) =: pad (|dy| <= 2e6).  With (*): py lies in
//   [min(y0, y1) - rho - pad, max(y0, y1) + rho + pad], and the step from py to j is the one from px to i above:
//   floor(lower) - 1 <= j <= floor(upper) + 2.
//  (A row whose T is empty has no member; whatever interval the clamped ends give there is harmless.)
struct SwingRows {
    int iLo, iHi;        // clamped to the map; iLo > iHi: nothing
    double padY;         // rho + pad
    double invDx, hw;    // fl(1 / dx) and rho * |fl(1 / dx)|, or invDx = 0: take the whole segment for every row
};
FPE_HD int swing_clamp_index(double lo, double v, double hi) { return static_cast<int>(fmin(fmax(v, lo), hi)); }
FPE_HD SwingRows swing_rows(const MapGeom& g, const SwingSeg& s, double r, double dx, double dy) {
    SwingRows w;
    const double rho = r + kSwingEta;
    const bool wide = fabs(dx) > fmax(2.0 * rho, g.res);
    w.invDx = wide ? 1.0 / dx : 0.0;
    w.hw = rho * fabs(w.invDx);
    w.padY = rho + kSwingEta * (1.0 + fabs(dy) * fabs(w.invDx));
    const double xmin = fmin(s.ax, s.bx), xmax = fmax(s.ax, s.bx);
    w.iLo = swing_clamp_index(0.0, floor((g.baseX - (xmax + rho)) * g.rinv) - 1.0, static_cast<double>(g.rows));
    w.iHi = swing_clamp_index(-1.0, floor((g.baseX - (xmin - rho)) * g.rinv) + 2.0, static_cast<double>(g.rows - 1));
    return w;
}
// dxa = px - ax
FPE_HD void swing_row_columns(const MapGeom& g, const SwingSeg& s, const SwingRows& w, double dy, double dxa, int& jLo,
                                                  int& jHi) {
    double tlo = 0.0, thi = 1.0;
    if (w.invDx != 0.0) {
        const double tm = dxa * w.invDx;
        tlo = fmin(fmax(tm - w.hw, 0.0), 1.0);
        thi = fmin(fmax(tm + w.hw, 0.0), 1.0);
    }
    const double y0 = s.ay + tlo * dy, y1 = s.ay + thi * dy;
    const double yLo = fmin(y0, y1) - w.padY, yHi = fmax(y0, y1) + w.padY;
    jLo = swing_clamp_index(0.0, floor((g.baseY - yHi) * g.rinv) - 1.0, static_cast<double>(g.cols));
    jHi = swing_clamp_index(-1.0, floor((g.baseY - yLo) * g.rinv) + 2.0, static_cast<double>(g.cols - 1));
}

// The record of one segment, computed by the sixteen lanes of its group (all of them active); every lane returns it.
__device__ __forceinline__ fpe_swing_record swing_segment_record(const DevMap& m, const SwingConsts& sc, const SwingSeg& s, int lane) {
    fpe_swing_record rec{};
    float rf;
    if (swing_refused(s, sc.defaultRadius, rf)) {
        rec.flags = FPE_SWING_REFUSED;
        return rec;
    }
    const MapGeom& g = m.g;
    const double r = static_cast<double>(rf), r2 = r * r;
    const double dx = s.bx - s.ax, dy = s.by - s.ay, L2 = dx * dx + dy * dy;
    const double rise = s.bz - s.az;
    const bool offMap = !(within_axis(s.ax, g.orgX, g.posX, g.lenX) && within_axis(s.ay, g.orgY, g.posY, g.lenY) &&
                          within_axis(s.bx, g.orgX, g.posX, g.lenX) && within_axis(s.by, g.orgY, g.posY, g.lenY));
    const SwingRows w = swing_rows(g, s, r, dx, dy);
    long long bestKey = kSwingNoKey64;  // no known member yet
    int bestCell = 0x7FFFFFFF;          // i * cols + j (below 2^30: check_map_geometry), so the lowest (row, column) is the lowest value
    int elevKey = kSwingNoKey32;
    int nCells = 0, nUnknown = 0;
    for (int i = w.iLo; i <= w.iHi; ++i) {
        const double px = cell_pos(g.baseX, g.res, i);
        const double dxa = px - s.ax;
        int jLo, jHi;
        swing_row_columns(g, s, w, dy, dxa, jLo, jHi);
        const double ux = dxa * dx;
        const int row0 = i * g.cols;
        for (int j = jLo + lane; j <= jHi; j += kSwingLanes) {
            const double py = cell_pos(g.baseY, g.res, j);
            double t = L2 > 0.0 ? (ux + (py - s.ay) * dy) / L2 : 0.0;
            t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
            const double ex = px - (s.ax + t * dx), ey = py - (s.ay + t * dy);
            if (ex * ex + ey * ey <= r2) {
                const float e = m.elev[row0 + j];
                ++nCells;
                if (isfinite(e) && e < 10.0f) {
                    const long long key = swing_key64(static_cast<double>(e) - (s.az + t * rise));
                    if (key > bestKey) {
                        bestKey = key;
                        bestCell = row0 + j;
                    }
                    elevKey = max(elevKey, swing_key32(e));
                } else {
                    ++nUnknown;
                }
            }
        }
    }
    // across the sixteen lanes: the maximum, then the lowest cell among the lanes that hold it
    const long long topKey = swing_max64(bestKey);
    const int cell = swing_min32(bestKey == topKey ? bestCell : 0x7FFFFFFF);
    elevKey = swing_max32(elevKey);
    nCells = swing_sum32(nCells);
    nUnknown = swing_sum32(nUnknown);
    const bool known = topKey != kSwingNoKey64;
    rec.lift = known ? swing_unkey64(topKey) : 0.0;
    rec.rise = rise;
    rec.length_sq = L2;
    rec.max_elevation = known ? swing_unkey32(elevKey) : 0.0f;
    rec.n_cells = nCells;
    rec.n_unknown = nUnknown;
    rec.row = known ? cell / g.cols : -1;
    rec.col = known ? cell % g.cols : -1;
    rec.flags = static_cast<uint8_t>(FPE_SWING_SEGMENT | (offMap ? FPE_SWING_OFF_MAP : 0u) | (nCells == 0 ? FPE_SWING_EMPTY : 0u) |
                                     (nUnknown > 0 ? FPE_SWING_UNKNOWN : 0u) | (rec.lift > sc.maxLift ? FPE_SWING_OVER_LIFT : 0u) |
                                     (fabs(rise) > sc.maxRise ? FPE_SWING_OVER_RISE : 0u) |
                                     (L2 > sc.maxLengthSq ? FPE_SWING_OVER_LENGTH : 0u));
    return rec;
}

// kPlan false: q[n] -> out[n].  kPlan true: n = B * nCycles * 4 segments from nominal, cycleOk and the start feet.
// Full occupancy: eight wavefronts per SIMD.
template <bool kPlan>
__global__ __launch_bounds__(256, 8) void swing_segments_kernel(DevMap m, SwingConsts sc, const fpe_swing_query* __restrict__ q,
                                                                const fpe_foothold* __restrict__ nominal,
                                                                const uint8_t* __restrict__ cycleOk, const double* __restrict__ startFeet,
                                                                int nCycles, int n, fpe_swing_record* __restrict__ out) {
    const int seg = static_cast<int>(blockIdx.x) * kSwingPerBlock + static_cast<int>(threadIdx.x) / kSwingLanes;
    const int lane = static_cast<int>(threadIdx.x) & (kSwingLanes - 1);
    if (seg >= n) return;  // (a whole group of sixteen lanes at a time: the shuffles below stay inside a group)
    SwingSeg s;
    fpe_swing_record rec{};
    if constexpr (kPlan) {
        const int leg = seg & 3, cyc = seg >> 2;  // cyc = b * nCycles + g
        const int g = cyc % nCycles, c0 = cyc - g;
        bool isSegment = cycleOk[cyc] != 0;
        if (isSegment) {
            const fpe_foothold to = nominal[seg];
            s.bx = to.x, s.by = to.y, s.bz = static_cast<double>(to.z);
            int gp = g - 1;  // the latest committed cycle before g: at most g bytes of cycle_ok
            while (gp >= 0 && cycleOk[c0 + gp] == 0) --gp;
            if (gp >= 0) {
                const fpe_foothold from = nominal[static_cast<size_t>(c0 + gp) * 4 + leg];
                s.ax = from.x, s.ay = from.y, s.az = static_cast<double>(from.z);
            } else {
                const double* f = startFeet + (static_cast<size_t>(c0 / nCycles) * 4 + leg) * 3;
                s.ax = f[0], s.ay = f[1], s.az = f[2];
            }
            s.radius = 0.0f;
            rec = swing_segment_record(m, sc, s, lane);
        }
        rec.foot_id = static_cast<uint8_t>(leg);
        rec.gait_cycle_id = static_cast<uint8_t>(g);
    } else {
        const fpe_swing_query qq = q[seg];
        s.ax = qq.a[0], s.ay = qq.a[1], s.az = qq.a[2];
        s.bx = qq.b[0], s.by = qq.b[1], s.bz = qq.b[2];
        s.radius = qq.radius;
        rec = swing_segment_record(m, sc, s, lane);
    }
    if (lane == 0) out[seg] = rec;
}

// Sixteen lanes per pose over its nCycles * 4 records (include/fpe.h: fpe_swing_summary)
__global__ __launch_bounds__(256, 8) void swing_summary_kernel(const fpe_swing_record* __restrict__ records, int B, int nCycles,
                                                               fpe_swing_summary* __restrict__ summary) {
    const int b = static_cast<int>(blockIdx.x) * kSwingPerBlock + static_cast<int>(threadIdx.x) / kSwingLanes;
    const int lane = static_cast<int>(threadIdx.x) & (kSwingLanes - 1);
    if (b >= B) return;
    const fpe_swing_record* __restrict__ rec = records + static_cast<size_t>(b) * nCycles * 4;
    constexpr uint32_t kOver = FPE_SWING_OVER_LIFT | FPE_SWING_OVER_RISE | FPE_SWING_OVER_LENGTH;
    constexpr uint32_t kUnknown = FPE_SWING_UNKNOWN | FPE_SWING_EMPTY | FPE_SWING_OFF_MAP;
    long long liftKey = kSwingNoKey64;
    long long riseKey = 0, lenKey = 0;  // fabs(rise) and length_sq are >= +0.0: their bit patterns order as integers
    int nSeg = 0, nOver = 0, nUnknown = 0, firstOver = 255;
    for (int k = lane; k < nCycles * 4; k += kSwingLanes) {
        const uint32_t f = rec[k].flags;
        if (!(f & FPE_SWING_SEGMENT)) continue;
        ++nSeg;
        liftKey = max(liftKey, swing_key64(rec[k].lift));
        riseKey = max(riseKey, __double_as_longlong(fabs(rec[k].rise)));
        lenKey = max(lenKey, __double_as_longlong(rec[k].length_sq));
        if (f & kOver) {
            ++nOver;
            firstOver = min(firstOver, k >> 2);
        }
        if (f & kUnknown) ++nUnknown;
    }
    liftKey = swing_max64(liftKey);
    riseKey = swing_max64(riseKey);
    lenKey = swing_max64(lenKey);
    nSeg = swing_sum32(nSeg);
    nOver = swing_sum32(nOver);
    nUnknown = swing_sum32(nUnknown);
    firstOver = swing_min32(firstOver);
    if (lane != 0) return;
    fpe_swing_summary s{};
    s.max_lift = nSeg > 0 ? swing_unkey64(liftKey) : 0.0;
    s.max_abs_rise = __longlong_as_double(riseKey);
    s.max_length_sq = __longlong_as_double(lenKey);
    s.n_segments = nSeg;
    s.n_over = nOver;
    s.n_unknown = nUnknown;
    s.first_over_cycle = static_cast<uint8_t>(firstOver);
    summary[b] = s;
}

}  // namespace

// res >= 1e-4 m and no cell farther than 2e6 m from the origin on either axis: what the proof at swing_row_columns assumes
bool swing_map_supported(const MapGeom& g) {
    return g.res >= 1e-4 && fabs(g.posX) + g.orgX <= 2e6 && fabs(g.posY) + g.orgY <= 2e6;
}

hipError_t launch_swing_segments(const DevMap& m, const SwingConsts& sc, const fpe_swing_query* d_q, int n, fpe_swing_record* d_out,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(swing_segments_kernel<false>, dim3((n + kSwingPerBlock - 1) / kSwingPerBlock), dim3(256), 0, stream, m, sc, d_q,
                       static_cast<const fpe_foothold*>(nullptr), static_cast<const uint8_t*>(nullptr), static_cast<const double*>(nullptr),
                       0, n, d_out);
    return hipGetLastError();
}

// d_records: B * nCycles * 4 records (required: the summary reads them); d_summary: B elements, or null
hipError_t launch_swing_plan(const DevMap& m, const SwingConsts& sc, const fpe_foothold* d_nominal, const uint8_t* d_cycleOk,
                             const double* d_startFeet, int B, int nCycles, fpe_swing_record* d_records, fpe_swing_summary* d_summary,
                             hipStream_t stream) {
    const int n = B * nCycles * 4;
    hipLaunchKernelGGL(swing_segments_kernel<true>, dim3((n + kSwingPerBlock - 1) / kSwingPerBlock), dim3(256), 0, stream, m, sc,
                       static_cast<const fpe_swing_query*>(nullptr), d_nominal, d_cycleOk, d_startFeet, nCycles, n, d_records);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !d_summary) return e;
    hipLaunchKernelGGL(swing_summary_kernel, dim3((B + kSwingPerBlock - 1) / kSwingPerBlock), dim3(256), 0, stream, d_records, B, nCycles,
                       d_summary);
    return hipGetLastError();
}
