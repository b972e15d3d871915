// fpe_beam.hpp — part nine of fpe_kernels.hip: beam search over stride options on resumable plans (fpe_plan_beam*, include/fpe.h).
// The kernels AROUND the resume kernels, which stay as they are: expand the surviving parents of every root into one candidate chain
// per option, (the engine launches the chained plan on those), score every candidate, keep the best n per root, remember their
// products and states, and — behind the last segment — follow the parent links back and write each final slot's path and products.
// No atomics anywhere: every output is a function of the inputs alone.  Candidate c = parent slot * M + option of root b is chain
// (b * nPrev + parent) * M + option of the segment's plan call: a root's keys are contiguous, its candidates compete only with each other.
#pragma once

namespace {

// `bytes` (a multiple of sizeof(Word)) from src to dst, one lane
template <class Word>
__device__ __forceinline__ void beam_copy_lane(void* dst, const void* src, int bytes) {
    const Word* s = static_cast<const Word*>(src);
    Word* d = static_cast<Word*>(dst);
    for (int i = 0; i < bytes / static_cast<int>(sizeof(Word)); ++i) d[i] = s[i];
}
template <class Word>
__device__ __forceinline__ void beam_expand_lane(const fpe_pose* pose, const fpe_stride* option, const fpe_plan_state* parent, fpe_pose* cp,
                                                 fpe_stride* cs, fpe_plan_state* cst) {
    beam_copy_lane<Word>(cp, pose, sizeof(fpe_pose));
    beam_copy_lane<Word>(cs, option, sizeof(fpe_stride));
    if (parent) beam_copy_lane<Word>(cst, parent, sizeof(fpe_plan_state));
}

// One lane per candidate chain: the root's pose, the option's stride and the parent's state into the dense arrays the plan call reads.
// parents: the caller's state_in (segment 0: one per root, parentStride 1, nPrev 1), the survivors' states of the previous segment
// (parentStride = the slot stride), or null (segment 0 from the poses: no state is written, the chain starts in the kernels' own
// prologue).  vec16: every source is 16-byte aligned (the destinations are scratch and always are).
__global__ __launch_bounds__(256) void beam_expand_kernel(const fpe_pose* __restrict__ poses, const fpe_stride* __restrict__ options,
                                                          const fpe_plan_state* __restrict__ parents, int parentStride, int nChains,
                                                          int nPrev, int M, fpe_pose* __restrict__ cp, fpe_stride* __restrict__ cs,
                                                          fpe_plan_state* __restrict__ cst, int vec16) {
    const int ch = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (ch >= nChains) return;
    const int m = ch % M, rp = ch / M;
    const int p = rp % nPrev, b = rp / nPrev;
    const fpe_plan_state* parent = parents ? parents + (static_cast<size_t>(b) * parentStride + p) : nullptr;
    if (vec16) beam_expand_lane<uint4>(poses + b, options + m, parent, cp + ch, cs + ch, cst + ch);
    else beam_expand_lane<uint2>(poses + b, options + m, parent, cp + ch, cs + ch, cst + ch);
}

// One candidate per group of four lanes, lane = leg (rank_summary_body's shape): the segment's penalty from its k cycles (the
// ranking's PenaltyAcc), the progress from the nominal track of its state_out, the score and the key.  Every lane of the group runs
// the same f64 chain in the stated order; lane 0 writes.  prevSurv: the previous segment's survivors (their penalty is the parent's), null in segment 0.
__global__ __launch_bounds__(256) void beam_score_kernel(int nChains, int nPrev, int M, int k, int slotStride, BeamConsts bc,
                                                         const fpe_foothold* __restrict__ nominal, const double* __restrict__ defaultNext,
                                                         const uint8_t* __restrict__ cycleOk, const fpe_plan_state* __restrict__ stateOut,
                                                         const BeamSurvivor* __restrict__ prevSurv, double* __restrict__ candPenalty,
                                                         double* __restrict__ candScore, RankKey* __restrict__ keys) {
    const int t = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    const int ch = t >> 2, leg = t & 3;
    const int cc = ch < nChains ? ch : nChains - 1;  // (lanes past the last chain run it again and write nothing: the shuffles stay whole)
    enum { RF = 0, RH = 1, LH = 2, LF = 3 };
    PenaltyAcc acc;
    const size_t rec0 = static_cast<size_t>(cc) * k * 4 + leg;
    for (int g = 0; g < k; ++g) {
        const size_t q = rec0 + static_cast<size_t>(g) * 4;
        acc.cycle(nominal[q], defaultNext + q * 3, cycleOk[static_cast<size_t>(cc) * k + g] != 0);
    }
    const double q = acc.finish(bc.wFail, bc.wSpiral, bc.wNone, bc.wDeviation, k);
    const double fx = stateOut[cc].feet[2][leg][0];
    double x[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) x[l] = __shfl(fx, l, 4);
    if (leg != 0 || ch >= nChains) return;
    const int nKeys = nPrev * M;
    const int c = ch % nKeys, b = ch / nKeys;
    const double parentPenalty = prevSurv ? prevSurv[static_cast<size_t>(b) * slotStride + c / M].penalty : 0.0;
    const double penalty = parentPenalty + q;
    const double cx = ((x[RF] + x[RH]) + (x[LH] + x[LF])) * 0.25;
    const double prog = bc.wProgress * cx;
    double sc = penalty - prog;
    if (sc == 0.0) sc = 0.0;  // -0.0 -> +0.0
    candPenalty[ch] = penalty;
    candScore[ch] = sc;
    keys[ch] = rank_key(sc, static_cast<uint32_t>(c), 0ull, 1ull);  // (class 1 falls to the candidate index alone)
}

constexpr int kBeamMaxKeys = FPE_BEAM_MAX_WIDTH * FPE_BEAM_MAX_OPTIONS;  // per root: 1024 keys, 16 KiB of LDS

// Workgroup blockIdx.x sorts root blockIdx.x's nKeys keys in LDS — the ranking's bitonic network (rank_sort_lds) over the next power of two,
// padded with "no candidate" keys — and writes the first nKeep as the segment's survivors, best first.
__global__ __launch_bounds__(256) void beam_select_kernel(const RankKey* __restrict__ keys, const double* __restrict__ candPenalty,
                                                          const double* __restrict__ candScore, int nKeys, int M, int nKeep, int slotStride,
                                                          BeamSurvivor* __restrict__ surv) {
    __shared__ RankKey s[kBeamMaxKeys];
    const int tid = static_cast<int>(threadIdx.x);
    const size_t base = static_cast<size_t>(blockIdx.x) * nKeys;
    int N = 2;
    while (N < nKeys) N <<= 1;
    const RankKey none{~0ull, ~0ull};
    for (int i = tid; i < N; i += 256) s[i] = i < nKeys ? keys[base + i] : none;
    __syncthreads();
    rank_sort_lds<256>(s, N, tid);
    for (int i = tid; i < nKeep; i += 256) {
        const int c = static_cast<int>(static_cast<uint32_t>(s[i].lo));
        BeamSurvivor v;
        v.parent = c / M;
        v.option = c % M;
        v.penalty = candPenalty[base + c];
        v.score = candScore[base + c];
        surv[static_cast<size_t>(blockIdx.x) * slotStride + i] = v;
    }
}

// Workgroup (root b, survivor w): the candidate's requested products into the segment's history slot [b][w] (cp.c[].dst is the
// segment's own part of the history), and its state_out into the next segment's parent array.
__global__ __launch_bounds__(256) void beam_keep_kernel(const BeamSurvivor* __restrict__ surv, int nPrev, int M, int nKeep, int slotStride,
                                                        RankCopies cp, const fpe_plan_state* __restrict__ stateOut,
                                                        fpe_plan_state* __restrict__ parents) {
    const int b = static_cast<int>(blockIdx.x) / nKeep, w = static_cast<int>(blockIdx.x) % nKeep;
    const size_t slot = static_cast<size_t>(b) * slotStride + w;
    const BeamSurvivor v = surv[slot];
    const size_t ch = (static_cast<size_t>(b) * nPrev + v.parent) * M + v.option;
    rank_copy_blocks(cp, ch, slot);
    constexpr int kWords = sizeof(fpe_plan_state) / sizeof(uint4);
    if (threadIdx.x < kWords)
        reinterpret_cast<uint4*>(parents + slot)[threadIdx.x] = reinterpret_cast<const uint4*>(stateOut + ch)[threadIdx.x];
}

// Workgroup (root b, final slot w): the parent links from the last segment back to the first — path[s], and segment s's history
// block to cycle offset s * k of the slot's products — then the slot's state, score and penalty; slot 0 also writes n_live[b].
// cp.c[].src: the whole history [S][B][slotStride] blocks; cp.c[].dst: the caller's product, [B][outStride][S] blocks.
__global__ __launch_bounds__(256) void beam_trace_kernel(const BeamSurvivor* __restrict__ surv, int B, int S, int nLive, int slotStride,
                                                         int outStride, RankCopies cp, const fpe_plan_state* __restrict__ parents,
                                                         int32_t* __restrict__ nLiveOut, double* __restrict__ score,
                                                         double* __restrict__ penalty, uint8_t* __restrict__ path,
                                                         fpe_plan_state* __restrict__ state) {
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
}

}  // namespace

int beam_live(const BeamShape& sh, int s) {
    long long n = 1;
    for (int q = 0; q <= s && n < sh.W; ++q) n *= sh.M;
    return static_cast<int>(n < sh.W ? n : sh.W);
}

hipError_t launch_beam_expand(const BeamShape& sh, int s, const fpe_pose* d_poses, const fpe_stride* d_options,
                              const fpe_plan_state* d_stateIn, const BeamScratch& sc, hipStream_t stream) {
    const int nPrev = s == 0 ? 1 : beam_live(sh, s - 1);
    const int nChains = sh.B * nPrev * sh.M;
    const fpe_plan_state* parents = s == 0 ? d_stateIn : sc.parents;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(d_poses) | reinterpret_cast<uintptr_t>(d_options) | reinterpret_cast<uintptr_t>(parents);
    hipLaunchKernelGGL(beam_expand_kernel, dim3((nChains + 255) / 256), dim3(256), 0, stream, d_poses, d_options, parents,
                       s == 0 ? 1 : sh.slotStride, nChains, nPrev, sh.M, sc.poses, sc.strides, sc.stateIn, (bits & 15) == 0 ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_beam_prune(const BeamConsts& bc, const BeamShape& sh, int s, const BeamScratch& sc, hipStream_t stream) {
    const int nPrev = s == 0 ? 1 : beam_live(sh, s - 1), nKeep = beam_live(sh, s);
    const int nChains = sh.B * nPrev * sh.M;
    const size_t segSlots = static_cast<size_t>(sh.B) * sh.slotStride;
    BeamSurvivor* surv = sc.surv + static_cast<size_t>(s) * segSlots;
    hipLaunchKernelGGL(beam_score_kernel, dim3(static_cast<unsigned>((static_cast<long long>(nChains) * 4 + 255) / 256)), dim3(256), 0, stream,
                       nChains, nPrev, sh.M, sh.k, sh.slotStride, bc, sc.cand.nominal, sc.cand.default_next, sc.cand.cycle_ok, sc.stateOut,
                       s == 0 ? nullptr : surv - segSlots, sc.candPenalty, sc.candScore, static_cast<RankKey*>(sc.keys));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_select_kernel, dim3(sh.B), dim3(256), 0, stream, static_cast<const RankKey*>(sc.keys), sc.candPenalty,
                       sc.candScore, nPrev * sh.M, sh.M, nKeep, sh.slotStride, surv);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_keep_kernel, dim3(sh.B * nKeep), dim3(256), 0, stream, surv, nPrev, sh.M, nKeep, sh.slotStride,
                       plan_copies(sc.cand, sc.hist, sh.k, static_cast<size_t>(s) * segSlots), sc.stateOut, sc.parents);
    return hipGetLastError();
}

hipError_t launch_beam_trace(const BeamShape& sh, const BeamScratch& sc, const fpe_beam_out& d_out, hipStream_t stream) {
    const int nLive = beam_live(sh, sh.S - 1);
    hipLaunchKernelGGL(beam_trace_kernel, dim3(sh.B * nLive), dim3(256), 0, stream, sc.surv, sh.B, sh.S, nLive, sh.slotStride, sh.outStride,
                       plan_copies(sc.hist, d_out.products, sh.k, 0), sc.parents, d_out.n_live, d_out.score, d_out.penalty, d_out.path,
                       d_out.state);
    return hipGetLastError();
}
