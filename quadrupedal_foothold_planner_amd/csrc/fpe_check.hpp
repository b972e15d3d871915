// fpe_check.hpp — part fourteen of the kernel translation unit (included last in fpe_kernels.hip, behind fpe_margin.hpp, inside
// namespace fpe): the checked ranking (fpe_plan_rank_checked*, fpe_check_plan_device, include/fpe.h) — every pose's plan reduced to
// the swing, trunk and margin summaries in registers, with no record array anywhere, and folded into the ranking's score and key.
//
// The arithmetic of the three checks exists once, in fpe_swing.hpp, fpe_trunk.hpp and fpe_margin.hpp: this file calls
// swing_segment_record, trunk_stance_record, margin_cell_refused / margin_row_nearest / margin_key / margin_record as they are and
// folds each returned record the way the three *_summary_kernels fold the stored ones (the same keys, the same neutral elements).
// Every summary field is a count, an extremum or an argmin with a stated tie rule, so it does not depend on how the items are dealt
// to the lanes: any mapping gives the same bytes.
//
//   plan_check_kernel<kRank>   ONE workgroup of four wavefronts per pose; no atomics, no scratch, 416 bytes of LDS for the
//                          hand-over.  A wavefront is four groups of sixteen lanes, the unit swing_segment_record and
//                          trunk_stance_record work in.  Each wavefront takes a share of every check, one behind the other:
//                          Swing: group `leg` walks its leg's chain of segments over the cycles in order and carries the last
//                          committed foothold in registers (the stored-record form searches cycle_ok backwards per segment);
//                          wavefront w computes the segments whose ordinal among the committed ones is w modulo 4 — the walk costs a
//                          32-byte load per cycle, the record is what is shared out.  cycle_ok is uniform in the workgroup, so the
//                          four groups stay in step.
//                          Trunk: the stances in chunks of four, one per group; chunk c goes to wavefront c modulo 4.
//                          Margin: the 4 n cells in sub-groups of 1 << margin_lanes_log2(reach) lanes, as margin_cells_kernel, in
//                          chunks of one wavefront's worth; chunk c goes to wavefront 3 - c modulo 4 — from the other end, so that at
//                          eight cycles two wavefronts hold the trunk's two chunks and the other two the margin's.
//                          A record comes back in EVERY lane of its group, so a group's accumulators are equal across its lanes and
//                          the sixteen-lane reductions of the summary kernels have nothing to do here: what remains is the combine
//                          ACROSS groups, xor shuffles at 16 and 32 (the margin: from the sub-group size up), after which every
//                          lane holds the wavefront's value.  A group without work skips only calls whose shuffles stay inside the
//                          group: no shuffle reads an idle lane.  Lane 0 of each wavefront puts its partial results into LDS; behind
//                          one barrier thread 0 merges the four (maxima, sums, minima), stores the summaries and finishes.
//                          kRank: behind rank_summary_kernel — reads its score[b] and gait_cycles_succeed, adds the check terms in
//                          the contract's order (-ffp-contract=off), writes base_score, score, hit and the key through rank_key.
//   Why not one wavefront per pose (the first mapping built, and measured): at 4 096 poses that is 4 096 wavefronts for the 1 024
//   SIMDs of the device — four per SIMD whatever the occupancy limit, the three checks one behind the other in each — where the
//   three stored-record kernels keep eight per SIMD busy.  It was 0.90 x the composed sequence on the headline map but 1.21 x on
//   4000 x 4000 at 0.5 cm, where a segment and a box cover 4 to 16 times the cells.  A wavefront per check (the swing on two) was
//   1.15 x there: the trunk's and the margin's wavefronts wait at the barrier, holding their slots, while the swing's finish
//   (profiles/rank_checked_summary.txt).
#pragma once

namespace {

// What a wavefront hands to thread 0: its part of the swing's and of the trunk's summary (three maxima as keys, three counts, the
// first flagged cycle) and of the margin's (the lowest key, three counts, the first cycle under the limit)
struct CheckPart {
    long long key[3];
    int count[3], first;
};
struct CheckMarginPart {
    long long best;
    int count[3], first;
};
struct CheckShared {
    CheckPart swing[4], trunk[4];
    CheckMarginPart margin[4];
};

// The combine across the groups of a wavefront: xor shuffles from offset `from` (the group size) up to 32
template <class T, class Op>
__device__ __forceinline__ T check_combine(T v, int from, Op op) {
    for (int o = from; o < 64; o <<= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ long long check_max64(long long v) {
    return check_combine(v, kSwingLanes, [](long long a, long long b) { return b > a ? b : a; });
}
__device__ __forceinline__ int check_sum32(int v, int from = kSwingLanes) {
    return check_combine(v, from, [](int a, int b) { return a + b; });
}
__device__ __forceinline__ int check_min32(int v, int from = kSwingLanes) {
    return check_combine(v, from, [](int a, int b) { return min(a, b); });
}

// Wavefront `wave` of the swing: the partial sums of fpe_swing_summary (as swing_summary_kernel forms it) over its segments
// (kWaves, here and below: the wavefronts that share a plan — four in plan_check_kernel; the checked beam also builds one)
template <int kWaves = 4>
__device__ __forceinline__ void check_swing_part(const DevMap& m, const CheckArgs& a, const fpe_foothold* __restrict__ nominal,
                                                 const uint8_t* __restrict__ ok, const double* __restrict__ feet, int nCycles, int wave,
                                                 int lane, CheckPart& out) {
    constexpr uint32_t kOver = FPE_SWING_OVER_LIFT | FPE_SWING_OVER_RISE | FPE_SWING_OVER_LENGTH;
    constexpr uint32_t kUnknown = FPE_SWING_UNKNOWN | FPE_SWING_EMPTY | FPE_SWING_OFF_MAP;
    const int leg = lane >> 4, l16 = lane & (kSwingLanes - 1);
    SwingSeg s;
    s.bx = feet[leg * 3], s.by = feet[leg * 3 + 1], s.bz = feet[leg * 3 + 2];  // the foot stands here
    s.radius = 0.0f;
    long long liftKey = kSwingNoKey64, riseKey = 0, lenKey = 0;
    int nSeg = 0, nOver = 0, nUnknown = 0, firstOver = 255;
    int ordinal = 0;
    for (int g = 0; g < nCycles; ++g) {
        if (ok[g] == 0) continue;  // (uniform in the workgroup)
        const fpe_foothold& to = nominal[g * 4 + leg];
        s.ax = s.bx, s.ay = s.by, s.az = s.bz;
        s.bx = to.x, s.by = to.y, s.bz = static_cast<double>(to.z);
        if ((ordinal++ & (kWaves - 1)) != wave) continue;  // another wavefront's segment
        const fpe_swing_record rec = swing_segment_record(m, a.sc, s, l16);
        const uint32_t fl = rec.flags;
        if (!(fl & FPE_SWING_SEGMENT)) continue;
        ++nSeg;
        liftKey = max(liftKey, swing_key64(rec.lift));
        riseKey = max(riseKey, __double_as_longlong(fabs(rec.rise)));
        lenKey = max(lenKey, __double_as_longlong(rec.length_sq));
        if (fl & kOver) {
            ++nOver;
            firstOver = min(firstOver, g);
        }
        if (fl & kUnknown) ++nUnknown;
    }
    liftKey = check_max64(liftKey);
    riseKey = check_max64(riseKey);
    lenKey = check_max64(lenKey);
    nSeg = check_sum32(nSeg);
    nOver = check_sum32(nOver);
    nUnknown = check_sum32(nUnknown);
    firstOver = check_min32(firstOver);
    if (lane != 0) return;
    out.key[0] = liftKey, out.key[1] = riseKey, out.key[2] = lenKey;
    out.count[0] = nSeg, out.count[1] = nOver, out.count[2] = nUnknown, out.first = firstOver;
}

// Wavefront `wave` of the trunk: the partial sums of fpe_trunk_summary (as trunk_summary_kernel forms it) over its stances
template <int kWaves = 4>
__device__ __forceinline__ void check_trunk_part(const DevMap& m, const CheckArgs& a, const fpe_foothold* __restrict__ nominal,
                                                 const uint8_t* __restrict__ ok, int nCycles, int wave, int lane, CheckPart& out) {
    constexpr uint32_t kBad = FPE_TRUNK_UNDER_CLEARANCE | FPE_TRUNK_OVER_SLOPE;
    constexpr uint32_t kUnknown = FPE_TRUNK_UNKNOWN | FPE_TRUNK_EMPTY | FPE_TRUNK_OFF_MAP;
    const int grp = lane >> 4, l16 = lane & (kSwingLanes - 1);
    long long clearKey = kSwingNoKey64, sxKey = 0, syKey = 0;
    int nStances = 0, nBad = 0, nUnknown = 0, firstBad = 255;
    for (int g = wave * 4 + grp; g < nCycles; g += 4 * kWaves) {
        if (ok[g] == 0) continue;  // (a whole group: trunk_stance_record's shuffles stay inside it)
        TrunkStance s;
#pragma unroll
        for (int leg = 0; leg < 4; ++leg) {
            const fpe_foothold& f = nominal[g * 4 + leg];
            s.x[leg] = f.x, s.y[leg] = f.y, s.z[leg] = static_cast<double>(f.z);
        }
        s.halfLength = s.halfWidth = 0.0f;
        const fpe_trunk_record rec = trunk_stance_record(m, a.tc, s, l16);
        const uint32_t fl = rec.flags;
        if (!(fl & FPE_TRUNK_STANCE)) continue;
        ++nStances;
        clearKey = max(clearKey, ~swing_key64(rec.clearance));
        sxKey = max(sxKey, __double_as_longlong(fabs(rec.slope_x)));
        syKey = max(syKey, __double_as_longlong(fabs(rec.slope_y)));
        if (fl & kBad) {
            ++nBad;
            firstBad = min(firstBad, g);
        }
        if (fl & kUnknown) ++nUnknown;
    }
    clearKey = check_max64(clearKey);
    sxKey = check_max64(sxKey);
    syKey = check_max64(syKey);
    nStances = check_sum32(nStances);
    nBad = check_sum32(nBad);
    nUnknown = check_sum32(nUnknown);
    firstBad = check_min32(firstBad);
    if (lane != 0) return;
    out.key[0] = clearKey, out.key[1] = sxKey, out.key[2] = syKey;
    out.count[0] = nStances, out.count[1] = nBad, out.count[2] = nUnknown, out.first = firstBad;
}

// Wavefront `wave` of the margin: the partial sums of fpe_margin_summary (as margin_summary_kernel forms it) over its cells
template <int kWaves = 4>
__device__ __forceinline__ void check_margin_part(const BitMap& bm, int rows, int cols, const CheckArgs& a,
                                                  const fpe_foothold* __restrict__ nominal, int nCycles, int wave, int lane,
                                                  CheckMarginPart& out) {
    const int reach = a.mc.reach;
    const int k = a.marginLanesLog2, L = 1 << k, sub = lane & (L - 1);
    const int nRec = nCycles * 4, per = 64 >> k;  // cells of a chunk
    long long best = 0x7FFFFFFFFFFFFFFFll;  // dist_sq << 16 | g * 4 + leg (below 2^32): the lowest (dist_sq, g, leg)
    int nFoot = 0, nUnder = 0, nOff = 0, firstUnder = 255;
    for (int s0 = (kWaves - 1 - wave) * per; s0 < nRec; s0 += kWaves * per) {
        const int s = s0 + (lane >> k);
        if (s >= nRec) continue;  // (a whole sub-group: the key's shuffles stay inside it — here and below)
        const fpe_foothold& f = nominal[s];
        if (f.valid == 0) continue;
        const int row = f.row, col = f.col;
        if (margin_cell_refused(rows, cols, row, col)) continue;  // FPE_MARGIN_REFUSED: no FOOTHOLD bit
        uint32_t key = kMarginNoKey;
        for (int di = sub - reach; di <= reach; di += L) {
            const int dj = margin_row_nearest(bm, rows, cols, a.mc.classes, row + di, col);
            if (dj != kMarginNoDj) key = min(key, margin_key(di, dj, reach));
        }
        for (int o = L >> 1; o > 0; o >>= 1) key = min(key, static_cast<uint32_t>(__shfl_xor(static_cast<int>(key), o)));
        const fpe_margin_record rec = margin_record(a.mc, rows, cols, row, col, key);
        ++nFoot;
        const long long kk = (static_cast<long long>(rec.dist_sq) << 16) | static_cast<long long>(s);
        best = kk < best ? kk : best;
        if (rec.flags & FPE_MARGIN_UNDER) {
            ++nUnder;
            firstUnder = min(firstUnder, s >> 2);
        }
        if (rec.flags & FPE_MARGIN_CENTRE_OFF_MAP) ++nOff;
    }
    best = check_combine(best, L, [](long long x, long long y) { return y < x ? y : x; });
    nFoot = check_sum32(nFoot, L);
    nUnder = check_sum32(nUnder, L);
    nOff = check_sum32(nOff, L);
    firstUnder = check_min32(firstUnder, L);
    if (lane != 0) return;
    out.best = best;
    out.count[0] = nFoot, out.count[1] = nUnder, out.count[2] = nOff, out.first = firstUnder;
}

// The four wavefronts' parts as one: maxima of the keys, sums of the counts, the lowest first cycle
__device__ __forceinline__ CheckPart check_merge(const CheckPart (&p)[4]) {
    CheckPart r = p[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            r.key[q] = max(r.key[q], p[w].key[q]);
            r.count[q] += p[w].count[q];
        }
        r.first = min(r.first, p[w].first);
    }
    return r;
}

// The grid is B workgroups: pose b = blockIdx.x
template <bool kRank>
__global__ __launch_bounds__(256) void plan_check_kernel(DevMap m, BitMap bm, CheckArgs a, int nCycles) {
    __shared__ CheckShared sh;
    const size_t b = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const fpe_foothold* __restrict__ nominal = a.nominal + b * nCycles * 4;
    const uint8_t* __restrict__ ok = a.cycleOk + b * nCycles;  // (not read by the margin)
    if (a.checks & FPE_CHECK_SWING) check_swing_part(m, a, nominal, ok, a.startFeet + b * 12, nCycles, wave, lane, sh.swing[wave]);
    if (a.checks & FPE_CHECK_TRUNK) check_trunk_part(m, a, nominal, ok, nCycles, wave, lane, sh.trunk[wave]);
    if (a.checks & FPE_CHECK_MARGIN) check_margin_part(bm, m.g.rows, m.g.cols, a, nominal, nCycles, wave, lane, sh.margin[wave]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    int unknown = 0, swingOver = 0, trunkBad = 0, marginUnder = 0;
    double maxLift = 0.0;
    if (a.checks & FPE_CHECK_SWING) {
        const CheckPart p = check_merge(sh.swing);
        maxLift = p.count[0] > 0 ? swing_unkey64(p.key[0]) : 0.0;
        swingOver = p.count[1];
        unknown += p.count[2];
        if (a.swing) {
            fpe_swing_summary o{};
            o.max_lift = maxLift;
            o.max_abs_rise = __longlong_as_double(p.key[1]);
            o.max_length_sq = __longlong_as_double(p.key[2]);
            o.n_segments = p.count[0];
            o.n_over = p.count[1];
            o.n_unknown = p.count[2];
            o.first_over_cycle = static_cast<uint8_t>(p.first);
            a.swing[b] = o;
        }
    }
    if (a.checks & FPE_CHECK_TRUNK) {
        const CheckPart p = check_merge(sh.trunk);
        trunkBad = p.count[1];
        unknown += p.count[2];
        if (a.trunk) {
            fpe_trunk_summary o{};
            o.min_clearance = p.count[0] > 0 ? swing_unkey64(~p.key[0]) : __longlong_as_double(0x7FF0000000000000ll);
            o.max_abs_slope_x = __longlong_as_double(p.key[1]);
            o.max_abs_slope_y = __longlong_as_double(p.key[2]);
            o.n_stances = p.count[0];
            o.n_bad = p.count[1];
            o.n_unknown = p.count[2];
            o.first_bad_cycle = static_cast<uint8_t>(p.first);
            a.trunk[b] = o;
        }
    }
    if (a.checks & FPE_CHECK_MARGIN) {
        CheckMarginPart p = sh.margin[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            p.best = min(p.best, sh.margin[w].best);
#pragma unroll
            for (int q = 0; q < 3; ++q) p.count[q] += sh.margin[w].count[q];
            p.first = min(p.first, sh.margin[w].first);
        }
        marginUnder = p.count[1];
        unknown += p.count[2];
        if (a.margin) {
            fpe_margin_summary o{};
            const int nFoot = p.count[0], kb = static_cast<int>(p.best & 0xFFFFll);
            o.min_dist_sq = nFoot > 0 ? static_cast<uint16_t>(p.best >> 16) : static_cast<uint16_t>(FPE_MARGIN_NONE);
            o.min_cycle = nFoot > 0 ? static_cast<uint8_t>(kb >> 2) : static_cast<uint8_t>(255);
            o.min_leg = nFoot > 0 ? static_cast<uint8_t>(kb & 3) : static_cast<uint8_t>(255);
            o.n_footholds = static_cast<uint16_t>(nFoot);
            o.n_under = static_cast<uint16_t>(p.count[1]);
            o.n_off_map = static_cast<uint16_t>(p.count[2]);
            o.first_under_cycle = static_cast<uint8_t>(p.first);
            a.margin[b] = o;
        }
    }
    const uint32_t hit = (swingOver > 0 ? FPE_CHECK_SWING : 0u) | (trunkBad > 0 ? FPE_CHECK_TRUNK : 0u) |
                         (marginUnder > 0 ? FPE_CHECK_MARGIN : 0u) | (unknown > 0 ? FPE_CHECK_UNKNOWN : 0u);
    if (a.hit) a.hit[b] = static_cast<uint8_t>(hit);
    if constexpr (kRank) {
        const double base = a.score[b];
        double v = base;
        if (a.checks & FPE_CHECK_SWING) {
            const double t0 = a.wSwingOver * static_cast<double>(swingOver);
            v = v + t0;
            const double t1 = a.wLift * maxLift;
            v = v + t1;
        }
        if (a.checks & FPE_CHECK_TRUNK) {
            const double t = a.wTrunkBad * static_cast<double>(trunkBad);
            v = v + t;
        }
        if (a.checks & FPE_CHECK_MARGIN) {
            const double t = a.wMarginUnder * static_cast<double>(marginUnder);
            v = v + t;
        }
        if (a.checks) {
            const double t = a.wUnknown * static_cast<double>(unknown);
            v = v + t;
        }
        if (v == 0.0) v = 0.0;  // -0.0 -> +0.0
        if (a.baseScore) a.baseScore[b] = base;
        a.score[b] = v;
        const bool cls1 = static_cast<int>(a.poseSummary[b].gait_cycles_succeed) < a.minCycles || (hit & a.reject) != 0u;
        static_cast<RankKey*>(a.keys)[b] = rank_key(v, static_cast<uint32_t>(b), cls1 ? 1ull : 0ull, 2ull);
    }
}

}  // namespace

hipError_t launch_plan_check(const CheckStage& st, int B, int nCycles, bool rank, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(B));
    if (rank) hipLaunchKernelGGL(plan_check_kernel<true>, grid, dim3(256), 0, stream, st.m, st.bm, st.a, nCycles);
    else hipLaunchKernelGGL(plan_check_kernel<false>, grid, dim3(256), 0, stream, st.m, st.bm, st.a, nCycles);
    return hipGetLastError();
}
