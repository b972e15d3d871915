// fpe_scan_close.hpp — part eighteen of the kernel translation unit (included at the end of fpe_kernels.hip, inside namespace fpe,
// behind fpe_scan_clear.hpp; it uses fpe_scan.hpp's constants): scan gap closing (fpe_scan_close*, include/fpe.h): the unknown cells
// of a rectangle of a state's elevation that lie between known cells take a height interpolated along the shortest spanning axis.
//
// A pure function of the elevation layer: the layer is only read, the result goes to the caller's rectangle-local buffers.  One
// launch per rectangle, in one of two forms of identical output:
//
//   scan_close_direct_kernel  one lane per cell of the rectangle.  A known cell costs one load and one store; an unknown cell walks
//                             the eight directions through global memory, each step checked against the map's edge.
//   scan_close_tiled_kernel   a workgroup of 256 lanes owns a 16 x 64 tile of the rectangle and stages it with a halo of `reach`
//                             cells in LDS (at most 32 x 80 words, 10 KB).  The halo is clamped to the MAP (not to the rectangle:
//                             the searches read the state around it); entries off the map hold NaN, and no load indexes outside
//                             the layer.  A wavefront takes one tile row at a time, lane = column: every LDS read of a wavefront,
//                             along a row, a column or a diagonal, touches consecutive words of one LDS row — no bank conflict at
//                             any pitch.  The searches run in LDS without an edge test.  The ROW axis is not searched at all: two
//                             ballots give the known bits of the wavefront's LDS row (64 tile columns, then the 2 x reach columns
//                             that remain of the halo), and s+ / s- of a lane are a count of trailing / leading zeros of its
//                             `reach` bits to either side (measured: 0.92 of the searched form's time on an ingest's rectangle,
//                             0.98 on the whole map; profiles/scan_close_summary.txt).
//
// Both share close_cell (the contract's steps 2-5 in f32, each operation rounded on its own: the translation unit is built without
// contraction) and the counting: a class's cells are counted by ballots into the workgroup's LDS words, the filled cells' bounding
// box by a wavefront reduction into LDS minima / maxima, and the workgroup issues ONE global atomic per non-zero counter.  The last
// workgroup (by ticket) takes the totals out with exchanges that leave the rest values and writes fpe_scan_close_info.  The
// accumulators are the close's own block (fpe_launch.hpp).  No float atomics, no per-cell atomics.
#pragma once

namespace {

constexpr int kCloseTileRows = 16;
constexpr int kCloseTileCols = 64;
constexpr int kClosePitch = kCloseTileCols + 2 * kCloseMaxReach;    // 80 words
constexpr int kCloseLdsRows = kCloseTileRows + 2 * kCloseMaxReach;  // 32 rows
static_assert(kScanBlock == 4 * kCloseTileCols, "four wavefronts, each a tile row wide");

__device__ __forceinline__ int32_t close_acc_rest(int w) {
    return (w == kCloseAccBox || w == kCloseAccBox + 1) ? INT32_MAX : (w == kCloseAccBox + 2 || w == kCloseAccBox + 3) ? -1 : 0;
}

// Steps 2-5 for an unknown cell -> its class (1 filled, 2 no_support, 3 rejected_axes, 4 rejected_spread) and the output's pattern.
// at(dr, dc): the height of the cell that far from this one, NaN where that lies off the map.
// rowSp >= 0: the row axis' s+ and s- are known already (0: none within reach) and are not searched.
template <class At>
__device__ __forceinline__ int close_cell(const ScanCloseArgs& a, At at, uint32_t& bits, int rowSp = -1, int rowSm = 0) {
    int n = 0, best = 1 << 30;
    float lo = __builtin_inff(), hi = -__builtin_inff(), v = 0.0f;
#pragma unroll
    for (int ax = 0; ax < 4; ++ax) {
        const int dr = ax == 0 ? 0 : 1;
        const int dc = ax == 1 ? 0 : ax == 3 ? -1 : 1;
        int sp = 0, sm = 0;
        float hp = 0.0f, hm = 0.0f;
        if (ax == 0 && rowSp >= 0) {
            if (rowSp == 0 || rowSm == 0) continue;
            sp = rowSp;
            sm = rowSm;
            hp = at(0, sp);
            hm = at(0, -sm);
        } else {
            for (int s = 1; s <= a.reach; ++s) {
                const float h = at(s * dr, s * dc);
                if (h == h) {
                    sp = s;
                    hp = h;
                    break;
                }
            }
            if (sp == 0) continue;
            for (int s = 1; s <= a.reach; ++s) {
                const float h = at(-s * dr, -s * dc);
                if (h == h) {
                    sm = s;
                    hm = h;
                    break;
                }
            }
            if (sm == 0) continue;
        }
        if (sp + sm - 1 > a.maxGap) continue;
        ++n;
        lo = fminf(lo, fminf(hp, hm));
        hi = fmaxf(hi, fmaxf(hp, hm));
        if (sp + sm < best) {  // (strictly: the lowest axis number among equals)
            best = sp + sm;
            v = hm + (hp - hm) * (static_cast<float>(sm) / static_cast<float>(sp + sm));
        }
    }
    bits = kScanCleared;
    if (n == 0) return 2;
    if (n < a.minAxes) return 3;
    if (!((hi - lo) <= a.maxSpread)) return 4;  // (a NaN difference, of inf - inf, lands here)
    if (v != v) return 4;
    bits = __float_as_uint(v);
    return 1;
}

// The workgroup's LDS words: sAcc[0..4] the classes' counts, sAcc[8..11] the filled cells' box.
__device__ __forceinline__ void close_acc_init(int32_t* sAcc) {
    if (threadIdx.x < 12) sAcc[threadIdx.x] = close_acc_rest(static_cast<int>(threadIdx.x));
}

// One cell per lane into the workgroup's words (cls < 0: the lane has no cell).  Every lane of the wavefront calls.
__device__ __forceinline__ void close_count(int32_t* sAcc, int cls, int i, int j) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned long long m = __ballot(cls == k);
        if (lane == 0 && m != 0ull) atomicAdd(sAcc + k, static_cast<int32_t>(__popcll(m)));
    }
    const bool filled = cls == 1;
    if (__ballot(filled) != 0ull) {  // (wave-uniform)
        int rmin = filled ? i : INT32_MAX, cmin = filled ? j : INT32_MAX, rmax = filled ? i : -1, cmax = filled ? j : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            rmin = min(rmin, __shfl_xor(rmin, d));
            cmin = min(cmin, __shfl_xor(cmin, d));
            rmax = max(rmax, __shfl_xor(rmax, d));
            cmax = max(cmax, __shfl_xor(cmax, d));
        }
        if (lane == 0) {
            atomicMin(sAcc + kCloseAccBox, rmin);
            atomicMin(sAcc + kCloseAccBox + 1, cmin);
            atomicMax(sAcc + kCloseAccBox + 2, rmax);
            atomicMax(sAcc + kCloseAccBox + 3, cmax);
        }
    }
}

// The workgroup's words into the state's accumulators, one atomic per non-zero counter; then the ticket, and the info from the last
// workgroup.  Every lane of the workgroup calls, once.
__device__ __forceinline__ void close_finish(const ScanCloseArgs& a, int32_t* sAcc, int32_t* sInfo, int32_t* sLast) {
    __syncthreads();
    const int w = static_cast<int>(threadIdx.x);
    if (w < 5) {
        if (sAcc[w]) atomicAdd(a.acc + w, sAcc[w]);
    } else if (w >= kCloseAccBox && w < kCloseAccBox + 4 && sAcc[1] != 0) {
        if (w < kCloseAccBox + 2) atomicMin(a.acc + w, sAcc[w]);
        else atomicMax(a.acc + w, sAcc[w]);
    }
    // (scan_fuse_kernel's ticket: this workgroup's atomics are performed before its ticket is drawn)
    __threadfence();
    __syncthreads();
    if (w == 0) *sLast = atomicAdd(reinterpret_cast<uint32_t*>(a.acc + kCloseTicket), 1u) == gridDim.x * gridDim.y - 1u;
    __syncthreads();
    if (!*sLast) return;
    __threadfence();
    if (w < 16) sInfo[w] = (w < 5 || (w >= kCloseAccBox && w < kCloseAccBox + 4)) ? atomicExch(a.acc + w, close_acc_rest(w)) : 0;
    if (w == 16) atomicExch(a.acc + kCloseTicket, 0);
    __syncthreads();
    if (w < 16 && a.info) {
        const int32_t cells = a.nr * a.nc;
        int32_t v = 0;
        if (w == 0) v = cells;
        else if (w == 1) v = sInfo[0];
        else if (w == 2) v = cells - sInfo[0];
        else if (w < 7) v = sInfo[w - 2];  // filled, no_support, rejected_axes, rejected_spread
        else if (w >= 8 && w < 12) v = sInfo[1] == 0 ? (w < 10 ? 0 : -1) : sInfo[w];  // no filled cell: {0, 0, -1, -1}
        a.info[w] = v;
    }
}

__global__ __launch_bounds__(kScanBlock) void scan_close_direct_kernel(ScanCloseArgs a) {
    __shared__ int32_t sAcc[12];
    __shared__ int32_t sInfo[16];
    __shared__ int32_t sLast;
    close_acc_init(sAcc);
    __syncthreads();
    const int idx = static_cast<int>(blockIdx.x) * kScanBlock + static_cast<int>(threadIdx.x);
    int cls = -1, i = 0, j = 0;
    if (idx < a.nr * a.nc) {
        const int r = idx / a.nc, c = idx - r * a.nc;
        i = a.row0 + r;
        j = a.col0 + c;
        uint32_t bits = a.elev[static_cast<size_t>(i) * static_cast<size_t>(a.cols) + static_cast<size_t>(j)];
        const float h = __uint_as_float(bits);
        if (h == h) {
            cls = 0;
        } else {
            cls = close_cell(
                a,
                [&](int dr, int dc) {
                    const int ii = i + dr, jj = j + dc;
                    if (ii < 0 || ii >= a.rows || jj < 0 || jj >= a.cols) return __uint_as_float(kScanCleared);
                    return __uint_as_float(a.elev[static_cast<size_t>(ii) * static_cast<size_t>(a.cols) + static_cast<size_t>(jj)]);
                },
                bits);
        }
        const size_t o = static_cast<size_t>(r) * static_cast<size_t>(a.outStride) + static_cast<size_t>(c);
        a.out[o] = bits;
        if (a.cls) a.cls[o] = static_cast<uint8_t>(cls);
    }
    close_count(sAcc, cls, i, j);
    close_finish(a, sAcc, sInfo, &sLast);
}

__global__ __launch_bounds__(kScanBlock) void scan_close_tiled_kernel(ScanCloseArgs a) {
    __shared__ uint32_t sTile[kCloseLdsRows * kClosePitch];
    __shared__ int32_t sAcc[12];
    __shared__ int32_t sInfo[16];
    __shared__ int32_t sLast;
    close_acc_init(sAcc);
    const int H = a.reach;  // 1 .. kCloseMaxReach (check_scan_close)
    const int tr0 = static_cast<int>(blockIdx.y) * kCloseTileRows, tc0 = static_cast<int>(blockIdx.x) * kCloseTileCols;  // rectangle-local
    const int ldsRows = kCloseTileRows + 2 * H, ldsCols = kCloseTileCols + 2 * H;
    for (int e = static_cast<int>(threadIdx.x); e < ldsRows * ldsCols; e += kScanBlock) {
        const int lr = e / ldsCols, lc = e - lr * ldsCols;
        const int gi = a.row0 + tr0 - H + lr, gj = a.col0 + tc0 - H + lc;
        uint32_t v = kScanCleared;
        if (gi >= 0 && gi < a.rows && gj >= 0 && gj < a.cols) v = a.elev[static_cast<size_t>(gi) * static_cast<size_t>(a.cols) + static_cast<size_t>(gj)];
        sTile[lr * kClosePitch + lc] = v;
    }
    __syncthreads();
    const int c = tc0 + (static_cast<int>(threadIdx.x) & 63);
    const int wave = static_cast<int>(threadIdx.x) >> 6;
#pragma unroll 1
    for (int p = 0; p < kCloseTileRows / 4; ++p) {
        const int r = tr0 + wave + 4 * p;
        int cls = -1;
        // the row's known bits from two ballots (every lane takes part: the row may lie below the rectangle, its LDS row exists):
        // lane l speaks for LDS column l, and the first 2 H lanes for the columns 64 .. 64 + 2 H - 1 as well
        const int lane = static_cast<int>(threadIdx.x) & 63;
        const uint32_t* row = sTile + (wave + 4 * p + H) * kClosePitch;
        const float f0 = __uint_as_float(row[lane]);
        const float f1 = lane < 2 * H ? __uint_as_float(row[kCloseTileCols + lane]) : __uint_as_float(kScanCleared);
        const unsigned __int128 known = (static_cast<unsigned __int128>(__ballot(f1 == f1)) << 64) | __ballot(f0 == f0);
        if (r < a.nr && c < a.nc) {
            const uint32_t* centre = sTile + (r - tr0 + H) * kClosePitch + (c - tc0 + H);
            uint32_t bits = *centre;
            const float h = __uint_as_float(bits);
            if (h == h) {
                cls = 0;
            } else {
                // this cell is LDS column x = lane + H: the columns x + 1 .. x + H above it, x - H .. x - 1 below it
                const uint32_t span = (1u << H) - 1u;
                const uint32_t up = static_cast<uint32_t>(known >> (lane + H + 1)) & span;
                const uint32_t down = static_cast<uint32_t>(known >> lane) & span;
                const int sp = up ? __builtin_ctz(up) + 1 : 0;
                const int sm = down ? H - (31 - __builtin_clz(down)) : 0;
                cls = close_cell(a, [&](int dr, int dc) { return __uint_as_float(centre[dr * kClosePitch + dc]); }, bits, sp, sm);
            }
            const size_t o = static_cast<size_t>(r) * static_cast<size_t>(a.outStride) + static_cast<size_t>(c);
            a.out[o] = bits;
            if (a.cls) a.cls[o] = static_cast<uint8_t>(cls);
        }
        close_count(sAcc, cls, a.row0 + r, a.col0 + c);
    }
    close_finish(a, sAcc, sInfo, &sLast);
}

__global__ void scan_close_reset_kernel(int32_t* acc) {
    const int k = static_cast<int>(threadIdx.x);
    if (k < kCloseAccWords) acc[k] = k < 16 ? close_acc_rest(k) : 0;
}

}  // namespace

hipError_t launch_scan_close(const ScanCloseArgs& a, int form, hipStream_t stream) {
    if (form == 1) {
        hipLaunchKernelGGL(scan_close_direct_kernel, dim3(scan_blocks(static_cast<size_t>(a.nr) * static_cast<size_t>(a.nc))), dim3(kScanBlock), 0, stream, a);
    } else {
        const dim3 grid(static_cast<unsigned>((a.nc + kCloseTileCols - 1) / kCloseTileCols), static_cast<unsigned>((a.nr + kCloseTileRows - 1) / kCloseTileRows));
        hipLaunchKernelGGL(scan_close_tiled_kernel, grid, dim3(kScanBlock), 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_scan_close_reset(int32_t* acc, hipStream_t stream) {
    hipLaunchKernelGGL(scan_close_reset_kernel, dim3(1), dim3(64), 0, stream, acc);
    return hipGetLastError();
}
