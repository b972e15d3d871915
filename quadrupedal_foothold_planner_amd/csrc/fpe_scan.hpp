// fpe_scan.hpp — part sixteen of the kernel translation unit (included at the end of fpe_kernels.hip, inside namespace fpe):
// scan fusion (fpe_scan_*, include/fpe.h): one point cloud scattered into the roi of a state's elevation and variance layers.
//
// Every per-cell reduction is an integer reduction (max of q, count and 64-bit sum of the kept q), so the layers do not depend on
// the order in which the points arrive or the atomics land.  No float atomics.  Three launches per fuse:
//
//   scan_top_kernel<merge>   one lane per point: the contract's per-point tests in f64 (the first failing test is the point's class),
//                            atomicMax of q into the cell's `top`, and an 8-byte record (local cell, q) for the next pass — the
//                            transform and the index division are not done twice.  The five classes are counted from ballots: one
//                            atomic per wavefront and class.
//   scan_sum_kernel<merge>   one lane per record: `top` of its cell decides kept (count + 1, sum + q: a 32-bit and a 64-bit integer
//                            atomic) or below the band (a ballot count).
//   scan_fuse_kernel         one lane per roi cell, lanes along a row: the cell's 16 scratch bytes in one load, the fusion rule in
//                            f32, both layers stored, the scratch put back to its rest value (no call starts with a memset), the cell
//                            classes from ballots and the bounding box from a wavefront reduction; the last workgroup to finish (a
//                            ticket) takes the totals out of the accumulators — atomic exchanges that leave the rest values behind —
//                            and writes the caller's fpe_scan_info.
//
// merge: neighbouring pixels of a depth image fall into the same cell, so adjacent lanes of a wavefront often hold equal cells.  The
// merged form numbers the runs of equal cells along the lanes, reduces each run in registers (six shuffle steps; integer max, or
// count and sum) and lets the run's first lane issue ONE atomic for it; the plain form issues one per point.  Same results.
//
// The state's own kernels: scan_move_kernel (both layers shifted by whole cells into the second buffer pair, cleared where nothing
// is carried), scan_set_kernel (both layers from two sources, unknown where either is NaN) and scan_reset_kernel (scratch and
// accumulators to their rest values, at create).
#pragma once

namespace {

constexpr int kScanBlock = 256;
constexpr uint32_t kScanCleared = 0x7FC00000u;  // the quiet NaN of an unknown cell (grid_map's cleared value)

// One atomic per wavefront for a class: the ballot's population, added by lane 0.  Every lane of the wavefront calls.
__device__ __forceinline__ void scan_count(bool p, int32_t* word, int lane) {
    const unsigned long long m = __ballot(p);
    if (lane == 0 && m != 0ull) atomicAdd(word, static_cast<int32_t>(__popcll(m)));
}

// Runs of equal keys along the lanes of the wavefront: whether this lane starts one, and the run's number (1-based, growing along
// the lanes, so two lanes are of one run iff their numbers are equal).  Every lane of the wavefront calls.
__device__ __forceinline__ bool scan_runs(uint32_t key, int lane, int& run) {
    const uint32_t prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    run = __popcll(heads & ((2ull << lane) - 1ull));  // heads at or below this lane (lane 63: the shift wraps to 0, the mask to all ones)
    return head;
}

// The contract's per-point tests (include/fpe.h, steps 1-6).  cls: 0 non-finite, 1 range, 2 height, 3 off the roi, 4 accepted.
struct ScanPoint {
    int32_t cls;
    uint32_t cell;  // local index in the roi, kScanNoCell unless accepted
    int32_t q;
};
__device__ __forceinline__ ScanPoint scan_classify(const ScanArgs& a, float x, float y, float z) {
    ScanPoint p{0, kScanNoCell, 0};
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) return p;
    const double xs = x, ys = y, zs = z;
    const double r2 = (xs * xs + ys * ys) + zs * zs;
    p.cls = 1;
    if (!(a.minR2 <= r2 && r2 <= a.maxR2)) return p;
    const double xm = ((a.T[0] * xs + a.T[1] * ys) + a.T[2] * zs) + a.T[3];
    const double ym = ((a.T[4] * xs + a.T[5] * ys) + a.T[6] * zs) + a.T[7];
    const double zm = ((a.T[8] * xs + a.T[9] * ys) + a.T[10] * zs) + a.T[11];
    p.cls = 2;
    if (!(a.minZ <= zm && zm <= a.maxZ)) return p;
    p.cls = 3;
    if (!(within_axis(xm, a.g.orgX, a.g.posX, a.g.lenX) && within_axis(ym, a.g.orgY, a.g.posY, a.g.lenY))) return p;
    const int ci = index_of(xm, a.g.orgX, a.g.posX, a.g.res) - a.row0;
    const int cj = index_of(ym, a.g.orgY, a.g.posY, a.g.res) - a.col0;
    if (ci < 0 || ci >= a.nr || cj < 0 || cj >= a.nc) return p;
    p.cls = 4;
    p.cell = static_cast<uint32_t>(ci * a.nc + cj);
    p.q = static_cast<int32_t>(rint(zm * 65536.0));  // |zm| <= 16384: |q| <= 2^30
    return p;
}

template <bool kMerge>
__global__ __launch_bounds__(kScanBlock) void scan_top_kernel(ScanArgs a) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int i = static_cast<int>(blockIdx.x) * kScanBlock + static_cast<int>(threadIdx.x);
    ScanPoint p{5, kScanNoCell, 0};  // (5: a lane behind the last point)
    if (i < a.n) {
        const float* s = a.points + static_cast<size_t>(i) * static_cast<size_t>(a.stride);
        p = scan_classify(a, s[0], s[1], s[2]);
        a.rec[i] = make_uint2(p.cell, static_cast<uint32_t>(p.q));
    }
    scan_count(p.cls == 0, a.acc + 1, lane);
    scan_count(p.cls == 1, a.acc + 2, lane);
    scan_count(p.cls == 2, a.acc + 3, lane);
    scan_count(p.cls == 3, a.acc + 4, lane);
    scan_count(p.cls == 4, a.acc + 5, lane);
    if (kMerge) {
        int run;
        const bool head = scan_runs(p.cell, lane, run);
        int32_t v = p.q;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t ov = __shfl_down(v, d);
            const int orun = __shfl_down(run, d);
            if (lane + d < 64 && orun == run) v = max(v, ov);
        }
        if (head && p.cell != kScanNoCell) atomicMax(&a.cells[p.cell].top, v);
    } else if (p.cell != kScanNoCell) {
        atomicMax(&a.cells[p.cell].top, p.q);
    }
}

template <bool kMerge>
__global__ __launch_bounds__(kScanBlock) void scan_sum_kernel(ScanArgs a) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int i = static_cast<int>(blockIdx.x) * kScanBlock + static_cast<int>(threadIdx.x);
    uint2 r = make_uint2(kScanNoCell, 0u);
    if (i < a.n) r = a.rec[i];
    const bool has = r.x != kScanNoCell;
    const int32_t q = static_cast<int32_t>(r.y);
    bool kept = false;
    if (has) kept = static_cast<int64_t>(q) >= static_cast<int64_t>(a.cells[r.x].top) - a.bandQ;
    scan_count(has && !kept, a.acc + 6, lane);
    if (kMerge) {
        int run;
        const bool head = scan_runs(r.x, lane, run);
        uint32_t cnt = kept ? 1u : 0u;
        long long sum = kept ? static_cast<long long>(q) : 0ll;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t oc = __shfl_down(cnt, d);
            const long long os = __shfl_down(sum, d);
            const int orun = __shfl_down(run, d);
            if (lane + d < 64 && orun == run) {
                cnt += oc;
                sum += os;
            }
        }
        if (head && cnt != 0u) {
            atomicAdd(&a.cells[r.x].count, cnt);
            atomicAdd(reinterpret_cast<unsigned long long*>(&a.cells[r.x].sum), static_cast<unsigned long long>(sum));
        }
    } else if (kept) {
        atomicAdd(&a.cells[r.x].count, 1u);
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.cells[r.x].sum), static_cast<unsigned long long>(static_cast<long long>(q)));
    }
}

__device__ __forceinline__ int32_t scan_acc_rest(int w) { return (w == 12 || w == 13) ? INT32_MAX : (w == 14 || w == 15) ? -1 : 0; }

__global__ __launch_bounds__(kScanBlock) void scan_fuse_kernel(ScanArgs a) {
    __shared__ int32_t sLast;
    __shared__ int32_t sInfo[16];
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int idx = static_cast<int>(blockIdx.x) * kScanBlock + static_cast<int>(threadIdx.x);
    const int total = a.nr * a.nc;
    int cls = 0;  // 0 not touched, 1 new, 2 fused, 3 outlier, 4 replaced
    int i = 0, j = 0;
    if (idx < total) {
        const int r = idx / a.nc;
        i = a.row0 + r;
        j = a.col0 + (idx - r * a.nc);
        const ScanCell sc = a.cells[idx];
        if (sc.count != 0u) {
            const float n = static_cast<float>(sc.count);
            const float zm = static_cast<float>((static_cast<double>(sc.sum) / static_cast<double>(sc.count)) * (1.0 / 65536.0));
            const double dx = cell_pos(a.g.baseX, a.g.res, i) - a.T[3];
            const double dy = cell_pos(a.g.baseY, a.g.res, j) - a.T[7];
            const float d2 = static_cast<float>(dx * dx + dy * dy);
            const float vm = fmaxf((a.varBase + a.varRange * d2) / n, a.varMin);
            const float vNew = fminf(vm, a.varMax);
            const size_t k = static_cast<size_t>(i) * static_cast<size_t>(a.g.cols) + static_cast<size_t>(j);
            const uint32_t hb = a.elev[k];
            const float h = __uint_as_float(hb), v = __uint_as_float(a.var[k]);
            float h2, v2;
            if (hb == kScanCleared) {
                cls = 1;
                h2 = zm;
                v2 = vNew;
            } else {
                const float d = zm - h, s = v + vm;
                if (d * d > a.gate2 * s) {
                    if (a.replaceCount > 0 && sc.count >= static_cast<uint32_t>(a.replaceCount)) {
                        cls = 4;
                        h2 = zm;
                        v2 = vNew;
                    } else {
                        cls = 3;
                        h2 = h;
                        v2 = fminf(v + a.varOutlier, a.varMax);
                    }
                } else {
                    cls = 2;
                    const float kk = v / s;
                    h2 = h + kk * d;
                    v2 = fminf(fmaxf(v - kk * v, a.varMin), a.varMax);
                }
            }
            uint32_t ho = __float_as_uint(h2), vo = __float_as_uint(v2);
            if (h2 != h2 || v2 != v2) ho = vo = kScanCleared;  // the invariant: unknown in both layers, one bit pattern
            a.elev[k] = ho;
            a.var[k] = vo;
            a.cells[idx] = ScanCell{kScanTopNone, 0u, 0};
        }
    }
    scan_count(cls != 0, a.acc + 7, lane);
    scan_count(cls == 1, a.acc + 8, lane);
    scan_count(cls == 2, a.acc + 9, lane);
    scan_count(cls >= 3, a.acc + 10, lane);
    scan_count(cls == 4, a.acc + 11, lane);
    if (__ballot(cls != 0) != 0ull) {  // (wave-uniform) the bounding box of the wavefront's touched cells: four atomics
        int rmin = cls ? i : INT32_MAX, cmin = cls ? j : INT32_MAX, rmax = cls ? i : -1, cmax = cls ? j : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            rmin = min(rmin, __shfl_xor(rmin, d));
            cmin = min(cmin, __shfl_xor(cmin, d));
            rmax = max(rmax, __shfl_xor(rmax, d));
            cmax = max(cmax, __shfl_xor(cmax, d));
        }
        if (lane == 0) {
            atomicMin(a.acc + 12, rmin);
            atomicMin(a.acc + 13, cmin);
            atomicMax(a.acc + 14, rmax);
            atomicMax(a.acc + 15, cmax);
        }
    }
    // The ticket: this workgroup's atomics are performed (fence) before its ticket is drawn; the workgroup that draws the last one
    // reads every total with an atomic exchange — the same coherence point the adds went to — which leaves the rest value behind.
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) sLast = atomicAdd(reinterpret_cast<uint32_t*>(a.acc + kScanTicket), 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!sLast) return;
    __threadfence();
    if (threadIdx.x < 16) sInfo[threadIdx.x] = atomicExch(a.acc + threadIdx.x, scan_acc_rest(static_cast<int>(threadIdx.x)));
    if (threadIdx.x == 16) atomicExch(a.acc + kScanTicket, 0);
    __syncthreads();
    if (threadIdx.x < 16 && a.info) {
        int32_t v = sInfo[threadIdx.x];
        if (threadIdx.x == 0) v = a.n;
        if (threadIdx.x >= 12 && sInfo[7] == 0) v = threadIdx.x < 14 ? 0 : -1;  // no touched cell: {0, 0, -1, -1}
        a.info[threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(kScanBlock) void scan_reset_kernel(ScanCell* cells, size_t n, int32_t* acc) {
    const size_t k = static_cast<size_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    if (k < n) cells[k] = ScanCell{kScanTopNone, 0u, 0};
    if (k < static_cast<size_t>(kScanAccWords)) acc[k] = k < 16 ? scan_acc_rest(static_cast<int>(k)) : 0;
}

__global__ __launch_bounds__(kScanBlock) void scan_move_kernel(const uint32_t* srcElev, const uint32_t* srcVar, uint32_t* dstElev, uint32_t* dstVar,
                                                               int rows, int cols, int sr, int sc) {
    const int j = static_cast<int>(blockIdx.x) * kScanBlock + static_cast<int>(threadIdx.x);
    const int i = static_cast<int>(blockIdx.y);
    if (j >= cols) return;
    const int si = i + sr, sj = j + sc;
    uint32_t e = kScanCleared, v = kScanCleared;
    if (si >= 0 && si < rows && sj >= 0 && sj < cols) {
        const size_t s = static_cast<size_t>(si) * cols + sj;
        e = srcElev[s];
        v = srcVar[s];
    }
    const size_t k = static_cast<size_t>(i) * cols + j;
    dstElev[k] = e;
    dstVar[k] = v;
}

__global__ __launch_bounds__(kScanBlock) void scan_set_kernel(const uint32_t* srcElev, const uint32_t* srcVar, uint32_t* dstElev, uint32_t* dstVar, size_t n) {
    const size_t k = static_cast<size_t>(blockIdx.x) * kScanBlock + threadIdx.x;
    if (k >= n) return;
    uint32_t e = kScanCleared, v = kScanCleared;
    if (srcElev) {
        e = srcElev[k];
        v = srcVar[k];
        const float ef = __uint_as_float(e), vf = __uint_as_float(v);
        if (ef != ef || vf != vf) e = v = kScanCleared;
    }
    dstElev[k] = e;
    dstVar[k] = v;
}

inline unsigned scan_blocks(size_t n) { return static_cast<unsigned>((n + kScanBlock - 1) / kScanBlock); }

}  // namespace

hipError_t launch_scan_top(const ScanArgs& a, bool merge, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    if (merge) hipLaunchKernelGGL(scan_top_kernel<true>, dim3(scan_blocks(static_cast<size_t>(a.n))), dim3(kScanBlock), 0, stream, a);
    else hipLaunchKernelGGL(scan_top_kernel<false>, dim3(scan_blocks(static_cast<size_t>(a.n))), dim3(kScanBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_scan_sum(const ScanArgs& a, bool merge, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    if (merge) hipLaunchKernelGGL(scan_sum_kernel<true>, dim3(scan_blocks(static_cast<size_t>(a.n))), dim3(kScanBlock), 0, stream, a);
    else hipLaunchKernelGGL(scan_sum_kernel<false>, dim3(scan_blocks(static_cast<size_t>(a.n))), dim3(kScanBlock), 0, stream, a);
    return hipGetLastError();
}

// (runs for n == 0 too: it writes the caller's info)
hipError_t launch_scan_cells(const ScanArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(scan_fuse_kernel, dim3(scan_blocks(static_cast<size_t>(a.nr) * static_cast<size_t>(a.nc))), dim3(kScanBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_scan_fuse(const ScanArgs& a, bool merge, hipStream_t stream) {
    hipError_t e = launch_scan_top(a, merge, stream);
    if (e == hipSuccess) e = launch_scan_sum(a, merge, stream);
    if (e == hipSuccess) e = launch_scan_cells(a, stream);
    return e;
}

hipError_t launch_scan_reset(ScanCell* cells, size_t n, int32_t* acc, hipStream_t stream) {
    hipLaunchKernelGGL(scan_reset_kernel, dim3(scan_blocks(n > static_cast<size_t>(kScanAccWords) ? n : kScanAccWords)), dim3(kScanBlock), 0, stream, cells, n, acc);
    return hipGetLastError();
}

hipError_t launch_scan_move(const uint32_t* srcElev, const uint32_t* srcVar, uint32_t* dstElev, uint32_t* dstVar, int rows, int cols, int sr, int sc,
                            hipStream_t stream) {
    hipLaunchKernelGGL(scan_move_kernel, dim3(scan_blocks(static_cast<size_t>(cols)), static_cast<unsigned>(rows)), dim3(kScanBlock), 0, stream, srcElev, srcVar,
                       dstElev, dstVar, rows, cols, sr, sc);
    return hipGetLastError();
}

hipError_t launch_scan_set(const uint32_t* srcElev, const uint32_t* srcVar, uint32_t* dstElev, uint32_t* dstVar, size_t n, hipStream_t stream) {
    hipLaunchKernelGGL(scan_set_kernel, dim3(scan_blocks(n)), dim3(kScanBlock), 0, stream, srcElev, srcVar, dstElev, dstVar, n);
    return hipGetLastError();
}
