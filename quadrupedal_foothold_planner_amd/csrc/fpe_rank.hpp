// fpe_rank.hpp — part seven of fpe_kernels.hip: rank a planned pose batch on the device (fpe_plan_rank*, include/fpe.h).
// Three kernels behind the plan kernel, on what it wrote: a per-pose summary with its score and sort key, the K smallest keys
// (sorted), and the copy of the chosen poses' products into K slots.  No atomics anywhere: every output is a function of the
// inputs alone.  The beam (fpe_beam.hpp) scores, sorts and copies with the same pieces, which live here once: PenaltyAcc, rank_key,
// rank_sort_lds, plan_copies / rank_copy_blocks.
#pragma once

// Sort key of one pose, ascending = better: hi = class << 32 | image >> 32, lo = image << 32 | pose index, with `image` the
// order-preserving 64-bit image of the score (0 for class 2: those fall to the index alone).  All ones = no pose.
struct alignas(16) RankKey {
    unsigned long long hi, lo;
};

constexpr int kRankTile = 8192;  // keys one workgroup sorts in LDS: 128 KiB of the CU's 160
constexpr int kRankMaxK = 1024;
constexpr int kRankProducts = kPlanProducts;  // (the product table: fpe_launch.hpp)

// One product of a block copy (a pose of the gather, a segment of a beam's keep / trace): `unit`-byte words (16, 4 or 1: what both
// pointers and the block size are multiples of)
struct RankCopy {
    const unsigned char* src;
    unsigned char* dst;
    uint32_t words;  // per block
    uint32_t unit;
};
struct RankCopies {
    RankCopy c[kRankProducts];
    int32_t n;
};

namespace {

__device__ __forceinline__ bool rank_key_less(const RankKey& a, const RankKey& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// The key of `score` (-0.0 already +0.0) and `index`: class `cls` and the order-preserving 64-bit image of the score, or — not
// finite — class `clsNonFinite` and no image: those fall to the index alone.
__device__ __forceinline__ RankKey rank_key(double score, uint32_t index, unsigned long long cls, unsigned long long clsNonFinite) {
    const bool finite = __builtin_isfinite(score);
    unsigned long long img = 0ull;
    if (finite) {
        const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(score));
        img = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
    }
    RankKey k;
    k.hi = ((finite ? cls : clsNonFinite) << 32) | (img >> 32);
    k.lo = (img << 32) | static_cast<unsigned long long>(index);
    return k;
}

// The penalty chain of one candidate — a ranked pose or a beam's chain — on its group of four lanes, lane = leg.  Every lane of
// the group runs the same f64 chain in the stated order (-ffp-contract=off): the scores are pinned byte for byte.
struct PenaltyAcc {
    uint32_t cnt01 = 0, cnt23 = 0;  // this leg's records by source, 16 bits each; behind finish(): the candidate's
    int committed = 0;
    double dev = 0.0;
    // One gait cycle: this leg's record `f`, its default_next (x, y, ..) and whether the cycle is committed (uniform within the
    // group: the shuffles run with every lane).
    __device__ __forceinline__ void cycle(const fpe_foothold& f, const double* __restrict__ defaultNext, bool ok) {
        enum { RF = 0, RH = 1, LH = 2, LF = 3 };
        const uint32_t src = f.source & 3u;
        const double dx = f.x - defaultNext[0], dy = f.y - defaultNext[1];
        const double term = dx * dx + dy * dy;
        if (src < 2) cnt01 += 1u << (16 * src);
        else cnt23 += 1u << (16 * (src - 2));
        double d[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) d[l] = __shfl(term, l, 4);
        if (!ok) return;
        ++committed;
        dev = dev + d[RF];
        dev = dev + d[RH];
        dev = dev + d[LH];
        dev = dev + d[LF];
    }
    __device__ __forceinline__ uint32_t n_source(int src) const { return ((src < 2 ? cnt01 : cnt23) >> (16 * (src & 1))) & 0xFFFFu; }
    // Behind the last of nCycles cycles: the source counts over the four legs, and the weighted sum in its fixed order.
    __device__ __forceinline__ double finish(double wFail, double wSpiral, double wNone, double wDeviation, int nCycles) {
        cnt01 += __shfl_xor(cnt01, 1, 4);
        cnt01 += __shfl_xor(cnt01, 2, 4);
        cnt23 += __shfl_xor(cnt23, 1, 4);
        cnt23 += __shfl_xor(cnt23, 2, 4);
        const double t0 = wFail * static_cast<double>(nCycles - committed);
        const double t1 = wSpiral * static_cast<double>(n_source(1));
        const double t2 = wNone * static_cast<double>(n_source(2) + n_source(3));
        const double t3 = wDeviation * dev;
        double q = t0 + t1;
        q = q + t2;
        q = q + t3;
        return q;
    }
};

// The bitonic network over s[0, N) in LDS (N a power of two, the keys in place and a barrier behind them), ascending, by the
// workgroup's kLanes lanes.  Declares no shared memory of its own: the kernels hand theirs.
template <int kLanes>
__device__ __forceinline__ void rank_sort_lds(RankKey* s, int N, int tid) {
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (N >> 1); i += kLanes) {
                const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), c = a | j;
                const RankKey ka = s[a], kc = s[c];
                const bool up = (a & k) == 0;
                if (rank_key_less(kc, ka) == up) {
                    s[a] = kc;
                    s[c] = ka;
                }
            }
            __syncthreads();
        }
    }
}

// One pose per group of four lanes, lane = leg: each lane loads its leg's records, the four values of a cycle meet by shuffle
// and every lane of the group runs the same f64 chain on them in the stated order (lane 0 writes).
// (the body of rank_summary_kernel and of its stride form — kStride: stepHalf is the pose's own, double(strides[b].step_length / 2))
template <bool kStride>
__device__ __forceinline__ void rank_summary_body(const fpe_pose* __restrict__ poses, int B, int nCycles, const RankConsts& rc,
                                                  const fpe_foothold* __restrict__ nominal, const double* __restrict__ defaultNext,
                                                  const uint8_t* __restrict__ cycleOk, const double* __restrict__ stance,
                                                  const uint8_t* __restrict__ poseStatus, fpe_pose_summary* __restrict__ summary,
                                                  double* __restrict__ score, RankKey* __restrict__ keys, const fpe_stride* __restrict__ strides) {
    const int t = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    const int b = t >> 2, leg = t & 3;
    const int bb = b < B ? b : B - 1;  // (lanes past the batch run pose B - 1 again and write nothing: the shuffles stay whole)
    int gait = leg == 0 ? poses[bb].gait : 0;
    gait = __shfl(gait, 0, 4);
    const bool trot = gait == 0;
    double stepHalf = rc.stepHalf;
    if constexpr (kStride) stepHalf = static_cast<double>(strides[bb].step_length / 2);
    const double cx = stance[static_cast<size_t>(bb) * 12 + leg * 3] - stepHalf;
    enum { RF = 0, RH = 1, LH = 2, LF = 3 };
    double cur[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) cur[l] = __shfl(cx, l, 4);
    PenaltyAcc acc;
    int succeed = 0, firstFailed = 255, lastOk = 0, nKpi = 0;
    double spSum = 0.0, spMin = 0.0, spMax = 0.0, fdMin = 0.0, fdMax = 0.0;
    const size_t rec0 = static_cast<size_t>(bb) * nCycles * 4 + leg;
    for (int g = 0; g < nCycles; ++g) {
        const size_t q = rec0 + static_cast<size_t>(g) * 4;
        const fpe_foothold& f = nominal[q];
        const double x = f.x;
        const int ok = cycleOk[static_cast<size_t>(bb) * nCycles + g] != 0;
        double r[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) r[l] = __shfl(x, l, 4);
        acc.cycle(f, defaultNext + q * 3, ok);
        lastOk = ok;
        if (!ok && firstFailed == 255) firstFailed = g;
        if (!ok) continue;  // (uniform within the pose's four lanes; the shuffles above ran with every lane)
        succeed = g + 1;
        if (trot) {  // assemble_track_report (fpe_host.cpp), nominal track
            const double fd0 = r[RF] - r[LH], fd1 = r[LF] - r[RH];
            double c1, c2, c3;
            if (rc.rfFirst) {
                c1 = (cur[RF] + cur[LH]) / 2;
                c2 = (r[LF] + r[RH]) / 2;
                c3 = (r[RF] + r[LH]) / 2;
            } else {
                c1 = (cur[LF] + cur[RH]) / 2;
                c2 = (r[RF] + r[LH]) / 2;
                c3 = (r[LF] + r[RH]) / 2;
            }
            const double s0 = (c2 - c1) / 0.5, s1 = (c3 - c2) / 0.5;
            if (nKpi == 0) {
                spMin = spMax = s0;
                fdMin = fdMax = fd0;
            }
            if (s0 < spMin) spMin = s0;
            if (s0 > spMax) spMax = s0;
            if (s1 < spMin) spMin = s1;
            if (s1 > spMax) spMax = s1;
            if (fd0 < fdMin) fdMin = fd0;
            if (fd0 > fdMax) fdMax = fd0;
            if (fd1 < fdMin) fdMin = fd1;
            if (fd1 > fdMax) fdMax = fd1;
            spSum = spSum + s0;
            spSum = spSum + s1;
            nKpi += 2;
#pragma unroll
            for (int l = 0; l < 4; ++l) cur[l] = r[l];
        }
    }
    double sc = acc.finish(rc.wFail, rc.wSpiral, rc.wNone, rc.wDeviation, nCycles);
    if (leg != 0 || b >= B) return;
    fpe_pose_summary s;
    s.success = static_cast<uint8_t>(lastOk);
    s.gait_cycles_succeed = static_cast<uint8_t>(succeed);
    s.committed = static_cast<uint8_t>(acc.committed);
    s.first_failed = static_cast<uint8_t>(firstFailed);
    s.pose_status = poseStatus[b];
    s.pad[0] = s.pad[1] = s.pad[2] = 0;
    for (int q = 0; q < 4; ++q) s.n_source[q] = static_cast<uint16_t>(acc.n_source(q));
    s.cog_speed_sum = spSum;
    s.cog_speed_min = spMin;
    s.cog_speed_max = spMax;
    s.feet_distance_min = fdMin;
    s.feet_distance_max = fdMax;
    s.deviation_sq_sum = acc.dev;
    summary[b] = s;
    const double t4 = rc.wSpeedSpread * (spMax - spMin);
    sc = sc + t4;
    if (sc == 0.0) sc = 0.0;  // -0.0 -> +0.0
    score[b] = sc;
    keys[b] = rank_key(sc, static_cast<uint32_t>(b), succeed < rc.minCycles ? 1ull : 0ull, 2ull);
}
__global__ __launch_bounds__(256) void rank_summary_kernel(const fpe_pose* __restrict__ poses, int B, int nCycles, RankConsts rc,
                                                           const fpe_foothold* __restrict__ nominal, const double* __restrict__ defaultNext,
                                                           const uint8_t* __restrict__ cycleOk, const double* __restrict__ stance,
                                                           const uint8_t* __restrict__ poseStatus, fpe_pose_summary* __restrict__ summary,
                                                           double* __restrict__ score, RankKey* __restrict__ keys) {
    rank_summary_body<false>(poses, B, nCycles, rc, nominal, defaultNext, cycleOk, stance, poseStatus, summary, score, keys, nullptr);
}
__global__ __launch_bounds__(256) void rank_summary_stride_kernel(const fpe_pose* __restrict__ poses, int B, int nCycles, RankConsts rc,
                                                                  const fpe_foothold* __restrict__ nominal, const double* __restrict__ defaultNext,
                                                                  const uint8_t* __restrict__ cycleOk, const double* __restrict__ stance,
                                                                  const uint8_t* __restrict__ poseStatus, fpe_pose_summary* __restrict__ summary,
                                                                  double* __restrict__ score, RankKey* __restrict__ keys,
                                                                  const fpe_stride* __restrict__ strides) {
    rank_summary_body<true>(poses, B, nCycles, rc, nominal, defaultNext, cycleOk, stance, poseStatus, summary, score, keys, strides);
}

// Workgroup blockIdx.x sorts keys [blockIdx.x * kRankTile, + kRankTile) of `in` (n keys in all) in LDS — a bitonic network over
// the next power of two, padded with "no pose" keys — and keeps the first K.  Tile stage (tileOut given): K keys per tile to
// tileOut, and (countsOut given) the tile's number of class-0 keys.  Final stage (one workgroup, n <= kRankTile): best[K], and
// n_class0 = the sum of `tileCounts` when a tile stage counted, else this workgroup's own count.
__global__ __launch_bounds__(1024) void rank_select_kernel(const RankKey* __restrict__ in, int n, int K, RankKey* __restrict__ tileOut,
                                                           int32_t* __restrict__ countsOut, int32_t* __restrict__ best,
                                                           int32_t* __restrict__ nClass0, const int32_t* __restrict__ tileCounts,
                                                           int nTileCounts) {
    extern __shared__ RankKey rankLds[];
    __shared__ int32_t waveCount[16];
    RankKey* s = rankLds;
    const int tid = static_cast<int>(threadIdx.x);
    const int base = static_cast<int>(blockIdx.x) * kRankTile;
    const int cnt = n - base < kRankTile ? n - base : kRankTile;
    int N = 64;
    while (N < cnt) N <<= 1;
    const RankKey none{~0ull, ~0ull};
    int c0 = 0;
    for (int i = tid; i < N; i += 1024) {
        RankKey k = none;
        if (i < cnt) {
            k = in[base + i];
            c0 += (k.hi >> 32) == 0ull;
        }
        s[i] = k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c0 += __shfl_xor(c0, o, 64);
    if ((tid & 63) == 0) waveCount[tid >> 6] = c0;
    __syncthreads();
    rank_sort_lds<1024>(s, N, tid);
    if (tileOut) {
        for (int i = tid; i < K; i += 1024) tileOut[static_cast<size_t>(blockIdx.x) * K + i] = i < N ? s[i] : none;
    } else {
        for (int i = tid; i < K; i += 1024) best[i] = static_cast<int32_t>(static_cast<uint32_t>(s[i].lo));
    }
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < 16; ++w) total += waveCount[w];
        if (countsOut) countsOut[blockIdx.x] = total;
        if (nClass0) {
            if (tileCounts) {
                total = 0;
                for (int q = 0; q < nTileCounts; ++q) total += tileCounts[q];
            }
            *nClass0 = total;
        }
    }
}

// Block `from` of one product to block `to`, word by word, by the workgroup's 256 lanes
template <class Word>
__device__ __forceinline__ void rank_copy_words(const RankCopy& c, size_t from, size_t to) {
    const Word* src = reinterpret_cast<const Word*>(c.src) + from * c.words;
    Word* dst = reinterpret_cast<Word*>(c.dst) + to * c.words;
    for (uint32_t i = threadIdx.x; i < c.words; i += 256) dst[i] = src[i];
}
// Block `from` of every product to block `to`
__device__ __forceinline__ void rank_copy_blocks(const RankCopies& cp, size_t from, size_t to) {
    for (int p = 0; p < cp.n; ++p) {
        const RankCopy& c = cp.c[p];
        if (c.unit == 16) rank_copy_words<uint4>(c, from, to);
        else if (c.unit == 4) rank_copy_words<uint32_t>(c, from, to);
        else rank_copy_words<unsigned char>(c, from, to);
    }
}
// Slot blockIdx.x takes pose best[blockIdx.x]: every requested product's block of that pose
__global__ __launch_bounds__(256) void rank_gather_kernel(const int32_t* __restrict__ best, RankCopies cp) {
    const size_t slot = blockIdx.x;
    rank_copy_blocks(cp, static_cast<size_t>(best[slot]), slot);
}

// The copies of the plan products both structs hold, from the product table: blocks of `cycles` gait cycles (one pose of a
// ranking, one segment of a beam), the destination's blocks counted from block dstBlockOffset.
inline RankCopies plan_copies(const fpe_plan_out& from, const fpe_plan_out& to, int cycles, size_t dstBlockOffset) {
    RankCopies cp;
    cp.n = 0;
    for (int k = 0; k < kPlanProducts; ++k) {
        const unsigned char* src = static_cast<const unsigned char*>(slots(from)[k]);
        unsigned char* dst = static_cast<unsigned char*>(slots(to)[k]);
        if (!src || !dst) continue;
        const size_t bytes = product_bytes(k, 1, static_cast<size_t>(cycles));
        const uintptr_t bits = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | bytes;
        const uint32_t unit = (bits & 15) == 0 ? 16u : ((bits & 3) == 0 ? 4u : 1u);
        cp.c[cp.n++] = RankCopy{src, dst + dstBlockOffset * bytes, static_cast<uint32_t>(bytes / unit), unit};
    }
    return cp;
}

inline size_t rank_align256(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }
inline int rank_tiles(int n) { return (n + kRankTile - 1) / kRankTile; }

}  // namespace

// Scratch of the ranking of B poses for the best K: the keys, then (B over one tile) the tile stages' two key buffers and the
// first stage's counts
size_t rank_scratch_bytes(int B, int K) {
    size_t total = rank_align256(static_cast<size_t>(B) * sizeof(RankKey));
    if (B > kRankTile) {
        const int t1 = rank_tiles(B);
        total += rank_align256(static_cast<size_t>(t1) * K * sizeof(RankKey));
        const long long n2 = static_cast<long long>(t1) * K;
        if (n2 > kRankTile) total += rank_align256(static_cast<size_t>(rank_tiles(static_cast<int>(n2))) * K * sizeof(RankKey));
        total += rank_align256(static_cast<size_t>(t1) * sizeof(int32_t));
    }
    return total;
}

// Summary, select and gather on `stream`, behind the plan kernel that wrote `full` (nominal, default_next, cycle_ok, stance and
// pose_status are read; a product of `bestProducts` is copied from the same product of `full`).  d_summary and d_score are
// required here (the engine hands scratch for what the caller did not ask for).
hipError_t launch_rank(const RankConsts& rc, const fpe_pose* d_poses, int B, int nCycles, int K, const fpe_plan_out& full,
                       fpe_pose_summary* d_summary, double* d_score, void* scratch, int32_t* d_best, int32_t* d_nClass0,
                       const fpe_plan_out& bestProducts, hipStream_t stream, const fpe_stride* d_strides, const CheckStage* check) {
    unsigned char* sp = static_cast<unsigned char*>(scratch);
    RankKey* keys = reinterpret_cast<RankKey*>(sp);
    sp += rank_align256(static_cast<size_t>(B) * sizeof(RankKey));
    const dim3 summaryGrid(static_cast<unsigned>((static_cast<long long>(B) * 4 + 255) / 256));
    if (d_strides)
        hipLaunchKernelGGL(rank_summary_stride_kernel, summaryGrid, dim3(256), 0, stream, d_poses, B, nCycles, rc, full.nominal, full.default_next,
                           full.cycle_ok, full.stance, full.pose_status, d_summary, d_score, keys, d_strides);
    else
        hipLaunchKernelGGL(rank_summary_kernel, summaryGrid, dim3(256), 0, stream,
                       d_poses, B, nCycles, rc, full.nominal, full.default_next, full.cycle_ok, full.stance, full.pose_status, d_summary,
                       d_score, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (check) {  // fpe_plan_rank_checked*: the check terms onto the summary's score, the keys rewritten (fpe_check.hpp)
        CheckStage st = *check;
        st.a.poseSummary = d_summary;
        st.a.score = d_score;
        st.a.keys = keys;
        st.a.minCycles = rc.minCycles;
        e = launch_plan_check(st, B, nCycles, true, stream);
        if (e != hipSuccess) return e;
    }
    const RankKey* cur = keys;
    int n = B;
    const int32_t* counts = nullptr;
    int nCounts = 0;
    if (B > kRankTile) {
        const int t1 = rank_tiles(B);
        RankKey* bufA = reinterpret_cast<RankKey*>(sp);
        sp += rank_align256(static_cast<size_t>(t1) * K * sizeof(RankKey));
        RankKey* bufB = reinterpret_cast<RankKey*>(sp);
        if (static_cast<long long>(t1) * K > kRankTile) sp += rank_align256(static_cast<size_t>(rank_tiles(t1 * K)) * K * sizeof(RankKey));
        int32_t* countsBuf = reinterpret_cast<int32_t*>(sp);
        RankKey* out = bufA;
        while (n > kRankTile) {  // every stage keeps K of each 8192 keys: at least four times fewer
            const int tiles = rank_tiles(n);
            hipLaunchKernelGGL(rank_select_kernel, dim3(tiles), dim3(1024), kRankTile * sizeof(RankKey), stream, cur, n, K, out,
                               counts ? nullptr : countsBuf, nullptr, nullptr, nullptr, 0);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
            if (!counts) {
                counts = countsBuf;
                nCounts = tiles;
            }
            cur = out;
            n = tiles * K;
            out = out == bufA ? bufB : bufA;
        }
    }
    int N = 64;
    while (N < n) N <<= 1;
    hipLaunchKernelGGL(rank_select_kernel, dim3(1), dim3(1024), N * sizeof(RankKey), stream, cur, n, K, nullptr, nullptr, d_best, d_nClass0,
                       counts, nCounts);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const RankCopies cp = plan_copies(full, bestProducts, nCycles, 0);
    if (cp.n == 0) return hipSuccess;
    hipLaunchKernelGGL(rank_gather_kernel, dim3(K), dim3(256), 0, stream, d_best, cp);
    return hipGetLastError();
}

hipError_t set_max_lds_rank() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(rank_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(kRankTile * sizeof(RankKey)));
}
