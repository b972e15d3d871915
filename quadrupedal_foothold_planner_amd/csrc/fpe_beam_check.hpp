// fpe_beam_check.hpp — part fifteen of the kernel translation unit (included behind fpe_check.hpp, inside namespace fpe): the checked
// beam (fpe_plan_beam_checked*, include/fpe.h) — the swing, trunk and margin checks folded into the beam's pruning.
//
// Three kernels beside the unchecked beam's five, which stay as they are (expand and select are launched unchanged):
//   beam_check_kernel<kWaves>  in the place of beam_score_kernel: one workgroup of kWaves wavefronts per candidate chain.  The
//                          segment's parts of the three summaries come from check_swing_part / check_trunk_part /
//                          check_margin_part (fpe_check.hpp) as they are — the arithmetic of a check exists once — on the
//                          candidate's k cycles, the swing starting from the PARENT's carried feet; wavefront 0 also runs the
//                          segment penalty (PenaltyAcc, beam_score_kernel's chain).  Behind one barrier thread 0 merges the parts
//                          with the parent's check state and writes the candidate's state, penalty, score and key.
//   beam_keep_checked_kernel   beam_keep_kernel's work plus the survivor's check state to the next segment's parents.
//   beam_trace_checked_kernel  beam_trace_kernel's work plus the final slot's state turned into the three summaries,
//                          base_penalty, hit and feet.
// The state is carried as KEYS AND COUNTS (CheckPart / CheckMarginPart), never as finished summaries: a summary's max_lift is 0
// without a segment while a real max_lift can be negative, and the margin's argmin key carries the global (cycle, leg).  Every
// field is a count, a maximum or a minimum of keys, so the state of a path is the exact merge of its segments' parts.  Cycle
// indices are made global (seg * k + g) in the merge: `first` fields and the low 16 bits of the margin's key.
// kWaves, both built and measured (profiles/beam_checked_summary.txt): 4 is plan_check_kernel's mapping, tuned for 8 cycles — at a
// segment's 2 one wavefront idles and two nearly do, holding their slots at the barrier: 1.09 x the composed sequence at 2 cm, 0.99 x
// at 0.5 cm.  1 runs the three checks one behind the other in one wavefront: 0.88 x at 2 cm, where a record covers a few hundred
// cells, 1.10 x at 0.5 cm, where a trunk box covers 3 080.  The engine picks by the cells under the body box (beam_check_map).
// No atomics, no scratch memory: every byte is a function of the inputs alone.
#pragma once

namespace {

// The check state of one candidate or parent: the path's parts so far, the unchecked accumulated penalty P_c (the only penalty a
// child inherits) and where the feet stand behind the path's last committed cycle.
struct BeamCheckState {
    CheckPart swing, trunk;
    CheckMarginPart margin;
    double penalty;
    double feet[12];
};
static_assert(sizeof(BeamCheckState) == kBeamCheckStateBytes && kBeamCheckStateBytes % 16 == 0, "BeamCheckState: the engine's size");

template <int kWaves>
struct BeamCheckShared {
    CheckPart swing[kWaves], trunk[kWaves];
    CheckMarginPart margin[kWaves];
    double q, cx;
};

constexpr long long kBeamNoMargin = 0x7FFFFFFFFFFFFFFFll;

// The part `p` of a segment whose first cycle is g0 onto the path's part `r`
__device__ __forceinline__ void beam_check_fold(CheckPart& r, const CheckPart& p, int g0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        r.key[q] = max(r.key[q], p.key[q]);
        r.count[q] += p.count[q];
    }
    if (p.first != 255) r.first = min(r.first, p.first + g0);
}

// Workgroup blockIdx.x = chain ch = (b * nPrev + parent) * M + option of the segment's plan call
template <int kWaves>
__global__ __launch_bounds__(64 * kWaves) void beam_check_kernel(DevMap m, BitMap bm, CheckArgs a, BeamCheckArgs ba) {
    __shared__ BeamCheckShared<kWaves> sh;
    const int ch = static_cast<int>(blockIdx.x);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int k = ba.k, nKeys = ba.nPrev * ba.M;
    const int c = ch % nKeys, b = ch / nKeys;
    const BeamCheckState* __restrict__ parent =
        ba.parents ? static_cast<const BeamCheckState*>(ba.parents) + (static_cast<size_t>(b) * ba.slotStride + c / ba.M) : nullptr;
    const double* __restrict__ rootFeet = ba.rootFeet ? ba.rootFeet + static_cast<size_t>(b) * ba.rootFeetStride : nullptr;
    const fpe_foothold* __restrict__ nominal = a.nominal + static_cast<size_t>(ch) * k * 4;
    const uint8_t* __restrict__ ok = a.cycleOk + static_cast<size_t>(ch) * k;
    if (a.checks & FPE_CHECK_SWING)  // (the host refuses a swing without any start feet: one of the two is given)
        check_swing_part<kWaves>(m, a, nominal, ok, parent ? parent->feet : rootFeet, k, wave, lane, sh.swing[wave]);
    if (a.checks & FPE_CHECK_TRUNK) check_trunk_part<kWaves>(m, a, nominal, ok, k, wave, lane, sh.trunk[wave]);
    if (a.checks & FPE_CHECK_MARGIN) check_margin_part<kWaves>(bm, m.g.rows, m.g.cols, a, nominal, k, wave, lane, sh.margin[wave]);
    if (wave == 0) {  // beam_score_kernel's chain, on every group of four lanes alike (lane & 3 = leg): lane 0 hands it over
        enum { RF = 0, RH = 1, LH = 2, LF = 3 };
        const int leg = lane & 3;
        PenaltyAcc acc;
        const size_t rec0 = static_cast<size_t>(ch) * k * 4 + leg;
        for (int g = 0; g < k; ++g) {
            const size_t q = rec0 + static_cast<size_t>(g) * 4;
            acc.cycle(a.nominal[q], ba.defaultNext + q * 3, ok[g] != 0);
        }
        const double q = acc.finish(ba.bc.wFail, ba.bc.wSpiral, ba.bc.wNone, ba.bc.wDeviation, k);
        const double fx = ba.stateOut[ch].feet[2][leg][0];
        double x[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) x[l] = __shfl(fx, l, 4);
        if (lane == 0) {
            sh.q = q;
            sh.cx = ((x[RF] + x[RH]) + (x[LH] + x[LF])) * 0.25;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    BeamCheckState st;
    if (parent) {
        st = *parent;
    } else {
        st.swing.key[0] = st.trunk.key[0] = kSwingNoKey64;
        st.swing.key[1] = st.swing.key[2] = st.trunk.key[1] = st.trunk.key[2] = 0;
        st.margin.best = kBeamNoMargin;
#pragma unroll
        for (int q = 0; q < 3; ++q) st.swing.count[q] = st.trunk.count[q] = st.margin.count[q] = 0;
        st.swing.first = st.trunk.first = st.margin.first = 255;
        st.penalty = 0.0;
#pragma unroll
        for (int q = 0; q < 12; ++q) st.feet[q] = rootFeet ? rootFeet[q] : 0.0;
    }
    const int g0 = ba.seg * k;
    if (a.checks & FPE_CHECK_SWING)
        for (int w = 0; w < kWaves; ++w) beam_check_fold(st.swing, sh.swing[w], g0);
    if (a.checks & FPE_CHECK_TRUNK)
        for (int w = 0; w < kWaves; ++w) beam_check_fold(st.trunk, sh.trunk[w], g0);
    if (a.checks & FPE_CHECK_MARGIN) {
        for (int w = 0; w < kWaves; ++w) {
            const CheckMarginPart p = sh.margin[w];
            if (p.count[0] > 0) st.margin.best = min(st.margin.best, p.best + static_cast<long long>(g0) * 4);  // (g * 4 + leg: global)
#pragma unroll
            for (int q = 0; q < 3; ++q) st.margin.count[q] += p.count[q];
            if (p.first != 255) st.margin.first = min(st.margin.first, p.first + g0);
        }
    }
    int last = -1;  // the carried feet: the latest committed cycle of the segment, else the parent's
    for (int g = 0; g < k; ++g)
        if (ok[g] != 0) last = g;
    if (last >= 0) {
#pragma unroll
        for (int leg = 0; leg < 4; ++leg) {
            const fpe_foothold& f = nominal[last * 4 + leg];
            st.feet[leg * 3] = f.x, st.feet[leg * 3 + 1] = f.y, st.feet[leg * 3 + 2] = static_cast<double>(f.z);
        }
    }
    st.penalty = st.penalty + sh.q;
    int unknown = 0;
    double v = st.penalty;
    uint32_t hit = 0u;
    if (a.checks & FPE_CHECK_SWING) {
        const int nOver = st.swing.count[1];
        const double maxLift = st.swing.count[0] > 0 ? swing_unkey64(st.swing.key[0]) : 0.0;
        const double t0 = a.wSwingOver * static_cast<double>(nOver);
        v = v + t0;
        const double t1 = a.wLift * maxLift;
        v = v + t1;
        unknown += st.swing.count[2];
        if (nOver > 0) hit |= FPE_CHECK_SWING;
    }
    if (a.checks & FPE_CHECK_TRUNK) {
        const double t = a.wTrunkBad * static_cast<double>(st.trunk.count[1]);
        v = v + t;
        unknown += st.trunk.count[2];
        if (st.trunk.count[1] > 0) hit |= FPE_CHECK_TRUNK;
    }
    if (a.checks & FPE_CHECK_MARGIN) {
        const double t = a.wMarginUnder * static_cast<double>(st.margin.count[1]);
        v = v + t;
        unknown += st.margin.count[2];
        if (st.margin.count[1] > 0) hit |= FPE_CHECK_MARGIN;
    }
    if (a.checks) {
        const double t = a.wUnknown * static_cast<double>(unknown);
        v = v + t;
    }
    if (unknown > 0) hit |= FPE_CHECK_UNKNOWN;
    const double prog = ba.bc.wProgress * sh.cx;
    double sc = v - prog;
    if (sc == 0.0) sc = 0.0;  // -0.0 -> +0.0
    static_cast<BeamCheckState*>(ba.cand)[ch] = st;
    ba.candPenalty[ch] = v;
    ba.candScore[ch] = sc;
    static_cast<RankKey*>(ba.keys)[ch] = rank_key(sc, static_cast<uint32_t>(c), (hit & a.reject) != 0u ? 1ull : 0ull, 2ull);
}

// beam_keep_kernel's work (the same text), and the survivor's check state into the next segment's parents
__global__ __launch_bounds__(256) void beam_keep_checked_kernel(const BeamSurvivor* __restrict__ surv, int nPrev, int M, int nKeep,
                                                                int slotStride, RankCopies cp, const fpe_plan_state* __restrict__ stateOut,
                                                                fpe_plan_state* __restrict__ parents,
                                                                const BeamCheckState* __restrict__ candCheck,
                                                                BeamCheckState* __restrict__ parentsCheck) {
    const int b = static_cast<int>(blockIdx.x) / nKeep, w = static_cast<int>(blockIdx.x) % nKeep;
    const size_t slot = static_cast<size_t>(b) * slotStride + w;
    const BeamSurvivor v = surv[slot];
    const size_t ch = (static_cast<size_t>(b) * nPrev + v.parent) * M + v.option;
    rank_copy_blocks(cp, ch, slot);
    constexpr int kWords = sizeof(fpe_plan_state) / sizeof(uint4), kCheckWords = sizeof(BeamCheckState) / sizeof(uint4);
    if (threadIdx.x < kWords)
        reinterpret_cast<uint4*>(parents + slot)[threadIdx.x] = reinterpret_cast<const uint4*>(stateOut + ch)[threadIdx.x];
    const int t = static_cast<int>(threadIdx.x) - 64;  // (the second wavefront)
    if (t >= 0 && t < kCheckWords) reinterpret_cast<uint4*>(parentsCheck + slot)[t] = reinterpret_cast<const uint4*>(candCheck + ch)[t];
}

// beam_trace_kernel's work (the same text), and the final slot's check state as the caller's check outputs: the summaries as
// plan_check_kernel finishes them from the same keys and counts
__global__ __launch_bounds__(256) void beam_trace_checked_kernel(const BeamSurvivor* __restrict__ surv, int B, int S, int nLive,
                                                                 int slotStride, int outStride, RankCopies cp,
                                                                 const fpe_plan_state* __restrict__ parents, int32_t* __restrict__ nLiveOut,
                                                                 double* __restrict__ score, double* __restrict__ penalty,
                                                                 uint8_t* __restrict__ path, fpe_plan_state* __restrict__ state,
                                                                 const BeamCheckState* __restrict__ parentsCheck, uint32_t checks,
                                                                 fpe_beam_check_out co) {
    const int b = static_cast<int>(blockIdx.x) / nLive, w = static_cast<int>(blockIdx.x) % nLive;
    const size_t out = static_cast<size_t>(b) * outStride + w;
    const size_t last = static_cast<size_t>(b) * slotStride + w;
    int slot = w;
    for (int s = S - 1; s >= 0; --s) {
        const size_t h = (static_cast<size_t>(s) * B + b) * slotStride + slot;
        const BeamSurvivor v = surv[h];
        if (threadIdx.x == 0) path[out * S + s] = static_cast<uint8_t>(v.option);
        rank_copy_blocks(cp, h, out * S + s);
        slot = v.parent;
    }
    constexpr int kWords = sizeof(fpe_plan_state) / sizeof(uint2);  // (the caller's array: 8-byte aligned by its type)
    if (state && threadIdx.x < kWords)
        reinterpret_cast<uint2*>(state + out)[threadIdx.x] = reinterpret_cast<const uint2*>(parents + last)[threadIdx.x];
    if (threadIdx.x == 0) {
        const BeamSurvivor v = surv[(static_cast<size_t>(S - 1) * B) * slotStride + last];
        if (score) score[out] = v.score;
        if (penalty) penalty[out] = v.penalty;
        if (nLiveOut && w == 0) nLiveOut[b] = nLive;
    }
    if (threadIdx.x != 64) return;  // (the second wavefront)
    const BeamCheckState st = parentsCheck[last];
    int unknown = 0;
    uint32_t hit = 0u;
    if (checks & FPE_CHECK_SWING) {
        const CheckPart& p = st.swing;
        unknown += p.count[2];
        if (p.count[1] > 0) hit |= FPE_CHECK_SWING;
        if (co.swing) {
            fpe_swing_summary o{};
            o.max_lift = p.count[0] > 0 ? swing_unkey64(p.key[0]) : 0.0;
            o.max_abs_rise = __longlong_as_double(p.key[1]);
            o.max_length_sq = __longlong_as_double(p.key[2]);
            o.n_segments = p.count[0];
            o.n_over = p.count[1];
            o.n_unknown = p.count[2];
            o.first_over_cycle = static_cast<uint8_t>(p.first);
            co.swing[out] = o;
        }
    }
    if (checks & FPE_CHECK_TRUNK) {
        const CheckPart& p = st.trunk;
        unknown += p.count[2];
        if (p.count[1] > 0) hit |= FPE_CHECK_TRUNK;
        if (co.trunk) {
            fpe_trunk_summary o{};
            o.min_clearance = p.count[0] > 0 ? swing_unkey64(~p.key[0]) : __longlong_as_double(0x7FF0000000000000ll);
            o.max_abs_slope_x = __longlong_as_double(p.key[1]);
            o.max_abs_slope_y = __longlong_as_double(p.key[2]);
            o.n_stances = p.count[0];
            o.n_bad = p.count[1];
            o.n_unknown = p.count[2];
            o.first_bad_cycle = static_cast<uint8_t>(p.first);
            co.trunk[out] = o;
        }
    }
    if (checks & FPE_CHECK_MARGIN) {
        const CheckMarginPart& p = st.margin;
        unknown += p.count[2];
        if (p.count[1] > 0) hit |= FPE_CHECK_MARGIN;
        if (co.margin) {
            fpe_margin_summary o{};
            const int nFoot = p.count[0], kb = static_cast<int>(p.best & 0xFFFFll);
            o.min_dist_sq = nFoot > 0 ? static_cast<uint16_t>(p.best >> 16) : static_cast<uint16_t>(FPE_MARGIN_NONE);
            o.min_cycle = nFoot > 0 ? static_cast<uint8_t>(kb >> 2) : static_cast<uint8_t>(255);
            o.min_leg = nFoot > 0 ? static_cast<uint8_t>(kb & 3) : static_cast<uint8_t>(255);
            o.n_footholds = static_cast<uint16_t>(nFoot);
            o.n_under = static_cast<uint16_t>(p.count[1]);
            o.n_off_map = static_cast<uint16_t>(p.count[2]);
            o.first_under_cycle = static_cast<uint8_t>(p.first);
            co.margin[out] = o;
        }
    }
    if (unknown > 0) hit |= FPE_CHECK_UNKNOWN;
    if (co.base_penalty) co.base_penalty[out] = st.penalty;
    if (co.hit) co.hit[out] = static_cast<uint8_t>(hit);
    if (co.feet) {
#pragma unroll
        for (int q = 0; q < 12; ++q) co.feet[out * 12 + q] = st.feet[q];
    }
}

}  // namespace

hipError_t launch_beam_prune_checked(const BeamShape& sh, int s, const BeamScratch& sc, const CheckStage& st, const BeamCheckArgs& args,
                                     int waves, hipStream_t stream) {
    const int nPrev = s == 0 ? 1 : beam_live(sh, s - 1), nKeep = beam_live(sh, s);
    const int nChains = sh.B * nPrev * sh.M;
    const size_t segSlots = static_cast<size_t>(sh.B) * sh.slotStride;
    BeamSurvivor* surv = sc.surv + static_cast<size_t>(s) * segSlots;
    BeamCheckArgs ba = args;
    ba.nPrev = nPrev, ba.M = sh.M, ba.k = sh.k, ba.slotStride = sh.slotStride, ba.seg = s;
    ba.defaultNext = sc.cand.default_next, ba.stateOut = sc.stateOut;
    ba.parents = s == 0 ? nullptr : sc.parentsCheck;
    if (s != 0) ba.rootFeet = nullptr;
    ba.cand = sc.candCheck, ba.candPenalty = sc.candPenalty, ba.candScore = sc.candScore, ba.keys = sc.keys;
    CheckArgs a = st.a;
    a.nominal = sc.cand.nominal, a.cycleOk = sc.cand.cycle_ok;
    if (waves == 1) hipLaunchKernelGGL(beam_check_kernel<1>, dim3(nChains), dim3(64), 0, stream, st.m, st.bm, a, ba);
    else hipLaunchKernelGGL(beam_check_kernel<4>, dim3(nChains), dim3(256), 0, stream, st.m, st.bm, a, ba);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_select_kernel, dim3(sh.B), dim3(256), 0, stream, static_cast<const RankKey*>(sc.keys), sc.candPenalty,
                       sc.candScore, nPrev * sh.M, sh.M, nKeep, sh.slotStride, surv);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_keep_checked_kernel, dim3(sh.B * nKeep), dim3(256), 0, stream, surv, nPrev, sh.M, nKeep, sh.slotStride,
                       plan_copies(sc.cand, sc.hist, sh.k, static_cast<size_t>(s) * segSlots), sc.stateOut, sc.parents,
                       static_cast<const BeamCheckState*>(sc.candCheck), static_cast<BeamCheckState*>(sc.parentsCheck));
    return hipGetLastError();
}

hipError_t launch_beam_trace_checked(const BeamShape& sh, const BeamScratch& sc, const fpe_beam_out& d_out, uint32_t checks,
                                     const fpe_beam_check_out& d_checkOut, hipStream_t stream) {
    const int nLive = beam_live(sh, sh.S - 1);
    hipLaunchKernelGGL(beam_trace_checked_kernel, dim3(sh.B * nLive), dim3(256), 0, stream, sc.surv, sh.B, sh.S, nLive, sh.slotStride,
                       sh.outStride, plan_copies(sc.hist, d_out.products, sh.k, 0), sc.parents, d_out.n_live, d_out.score, d_out.penalty,
                       d_out.path, d_out.state, static_cast<const BeamCheckState*>(sc.parentsCheck), checks, d_checkOut);
    return hipGetLastError();
}
