// fpe_footmap.hpp — part four of the kernel translation unit (included at the end of fpe_kernels.hip, inside
// namespace fpe): the dense foothold map (fpe_foothold_map*, include/fpe.h).
//
// For every cell (i, j) of a region of the snapshot, the reference's own disc functions evaluated at the cell centre
// p = getPosition(i, j), disc = CircleIterator(map, p, footRadius):
//   * FPE_FMAP_DEFAULT_OK   checkDefaultFoothold (cpp:2039-2082): no FINITE cell of the disc below defaultFootholdThreshold_;
//   * FPE_FMAP_CANDIDATE_OK checkCirclePolygonFoothold (cpp:2117-2163) with a polygon that holds every cell: the same with
//                           candidateFootholdThreshold_ (exactly the spiral candidate test of the plan kernels);
//   * FPE_FMAP_UNKNOWN      some in-map cell of the disc has non-finite traversability (build-defined);
//   * height                getFootholdMeanHeight (cpp:2520-2554): the ordered f32 sum, finish_mean.
// A cell-centred disc always holds its own cell (squared distance 0), so "the disc is non-empty" holds for every in-map
// cell; the literal walk still tracks it.
//
// Three kernels, chosen on the host (launch_foothold_map):
//   footmap_flags_bits_kernel  the flags of a host-proved disc with a row-interval form (PlanConsts::footRobust, nHW > 0):
//                              a bitwise dilation of the planes Df, C and (~F & in-map) by the disc's row intervals, one
//                              lane per 32-cell word, on the tiled planes (8 lanes = the 8 rows of one 128-byte line);
//   footmap_height_kernel      the heights of a host-proved disc: an elevation tile plus a halo of footReach in LDS, one
//                              lane per column of eight cells, the ordered offset table walked in order;
//   footmap_direct_kernel      one lane per cell on the f32 layers: the literal f64 CircleIterator walk (discs that fail the
//                              proof, or fpe_set_tuning("literal_discs", 1)) — flags and heights — or, for a proved disc
//                              without a row-interval form, the flags over the offset table.
#pragma once

// The literal walk visits a (2 ceil(rf / res) + 2)^2 box per cell: bounded so that one call stays a short kernel
constexpr int kFmapMaxLiteralReach = 32;

namespace {

constexpr int kFmapRows = 8;    // flag kernel: rows per workgroup (the 8 rows of one tiled line)
constexpr int kFmapWords = 32;  // flag kernel: words per workgroup (1024 columns)
constexpr int kHmapRows = 32;   // height kernel: output tile of 32 rows x 64 columns, a column of 8 cells per lane
constexpr int kHmapCols = 64;
constexpr int kHmapMaxReach = 7;  // a proved table has at most kMaxFootOffsets = 128 cells: footReach <= 6
constexpr int kHmapTileW = kHmapCols + 2 * kHmapMaxReach;
constexpr int kHmapTileH = kHmapRows + 2 * kHmapMaxReach;

// Horizontal dilation of word `cur` by the columns [-hw, hw], hw <= 15: bit b of the result is set iff some bit b + d,
// |d| <= hw, of the 96-bit row prev | cur | next is set (bit b of a word = column 32 w + b).
__device__ __forceinline__ uint32_t fmap_hdilate(uint32_t prev, uint32_t cur, uint32_t next, int hw) {
    const uint64_t hi = (static_cast<uint64_t>(next) << 32) | cur;
    const uint64_t lo = (static_cast<uint64_t>(cur) << 32) | prev;
    uint32_t r = cur;
    for (int d = 1; d <= hw; ++d) r |= static_cast<uint32_t>(hi >> d) | static_cast<uint32_t>(lo >> (32 - d));
    return r;
}

// In-map columns of word ww
__device__ __forceinline__ uint32_t fmap_col_mask(int ww, int cols) {
    const int n = cols - 32 * ww;
    if (ww < 0 || n <= 0) return 0u;
    return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);
}

__global__ __launch_bounds__(256) void footmap_flags_bits_kernel(BitMap bm, int rows, int cols, PlanConsts pc, FootmapRoi roi,
                                                                 uint8_t* __restrict__ flags) {
    __shared__ uint32_t stage[kFmapRows][kFmapWords * 8];  // the block's flag bytes, row by row
    const int t = static_cast<int>(threadIdx.x);
    const int r = t & 7, wl = t >> 3;
    const int wBase = (roi.col0 >> 5) + static_cast<int>(blockIdx.x) * kFmapWords;
    const int iBase = roi.row0 + static_cast<int>(blockIdx.y) * kFmapRows;
    const int w = wBase + wl, i = iBase + r;
    const int lastW = (roi.col0 + roi.nc - 1) >> 5, lastI = roi.row0 + roi.nr - 1;
    uint32_t dDf = 0u, dC = 0u, dU = 0u;  // dilations: some disc cell has Df / C / unknown traversability
    if (w <= lastW && i <= lastI) {
        const uint32_t mP = fmap_col_mask(w - 1, cols), mC = fmap_col_mask(w, cols), mN = fmap_col_mask(w + 1, cols);
        const int R = pc.footReach;
        for (int a = -R; a <= R; ++a) {
            // rows -1 and `rows` of the planes are zero: a disc row beyond them reads the nearest one
            const int q = min(max(i + a, -1), rows);
            const uint32_t rowIn = (q >= 0 && q < rows) ? 0xFFFFFFFFu : 0u;
            const uint4 gp = bm.words[bit_group_index(q, w - 1, bm.strideW)];
            const uint4 gc = bm.words[bit_group_index(q, w, bm.strideW)];
            const uint4 gn = bm.words[bit_group_index(q, w + 1, bm.strideW)];
            const int hw = pc.hwList[pc.hwIdx[a < 0 ? -a : a]];
            dDf |= fmap_hdilate(gp.y, gc.y, gn.y, hw);
            dC |= fmap_hdilate(gp.z, gc.z, gn.z, hw);
            dU |= fmap_hdilate(~gp.w & mP & rowIn, ~gc.w & mC & rowIn, ~gn.w & mN & rowIn, hw);
        }
    }
    // widen to one flag byte per cell
    const uint32_t okD = ~dDf, okC = ~dC;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t v = 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = 4 * k + u;
            const uint32_t f = ((okD >> b) & 1u) | (((okC >> b) & 1u) << 1) | (((dU >> b) & 1u) << 2);
            v |= f << (8 * u);
        }
        stage[r][wl * 8 + k] = v;
    }
    __syncthreads();
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(&stage[0][0]);
    const int colBase = 32 * wBase;
    for (int k = t; k < kFmapRows * kFmapWords * 32; k += 256) {
        const int rr = k >> 10, cc = k & 1023;
        const int ii = iBase + rr, jj = colBase + cc;
        if (ii <= lastI && jj >= roi.col0 && jj < roi.col0 + roi.nc)
            flags[static_cast<size_t>(ii - roi.row0) * roi.nc + (jj - roi.col0)] = sb[k];
    }
}

__global__ __launch_bounds__(256) void footmap_height_kernel(DevMap m, PlanConsts pc, FootmapRoi roi, float* __restrict__ height) {
    // elevation values as getFootholdMeanHeight reads them (non-finite -> 0, cpp:2532-2537); NaN marks "not in the map"
    __shared__ float tile[kHmapTileH * kHmapTileW];
    __shared__ int offs[kMaxFootOffsets];
    const int t = static_cast<int>(threadIdx.x);
    const int R = pc.footReach;
    const int iBase = roi.row0 + static_cast<int>(blockIdx.y) * kHmapRows, jBase = roi.col0 + static_cast<int>(blockIdx.x) * kHmapCols;
    const int th = kHmapRows + 2 * R, tw = kHmapCols + 2 * R;
    for (int k = t; k < th * tw; k += 256) {
        const int a = k / tw, b = k - a * tw;
        const int i = iBase - R + a, j = jBase - R + b;
        float v = __builtin_nanf("");
        if (in_range(i, j, m.g.rows, m.g.cols)) {
            const float e = m.elev[static_cast<size_t>(i) * m.g.cols + j];
            v = __builtin_isfinite(e) ? e : 0.0f;
        }
        tile[a * kHmapTileW + b] = v;
    }
    for (int k = t; k < pc.nFoot; k += 256) offs[k] = pc.footDa[k] * kHmapTileW + pc.footDb[k];
    __syncthreads();
    const int tx = t & 63, ty = t >> 6;
    const float* base = tile + (ty * 8 + R) * kHmapTileW + tx + R;
    float sum[8], last[8];
    int cnt[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        sum[u] = 0.0f;
        last[u] = 0.0f;
        cnt[u] = 0;
    }
    // the offset table is row-major from the smallest index: the CircleIterator order (cpp:2539-2545); one plain f32 add per
    // visited cell below 10 (cells outside the map hold NaN: never below 10).  A skipped cell adds -0.0f, which leaves every
    // sum bit for bit as it is (round to nearest; the sum starts at +0.0f): no branch in the loop.
    for (int k = 0; k < pc.nFoot; ++k) {
        const int o = offs[k];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float e = base[u * kHmapTileW + o];
            const bool take = e < 10.0f;
            sum[u] = sum[u] + (take ? e : -0.0f);
            cnt[u] += take ? 1 : 0;
        }
    }
    const int j = jBase + tx;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = iBase + ty * 8 + u;
        if (cnt[u] == 0) {  // no height below 10 (cpp:2547-2551): the last visited cell's value, the last in-map table entry
            for (int k = pc.nFoot - 1; k >= 0; --k) {
                const float e = base[u * kHmapTileW + offs[k]];
                if (e == e) {
                    last[u] = e;
                    break;
                }
            }
        }
        if (i < roi.row0 + roi.nr && j < roi.col0 + roi.nc)
            height[static_cast<size_t>(i - roi.row0) * roi.nc + (j - roi.col0)] = finish_mean(sum[u], last[u], cnt[u], pc.h);
    }
}

// One lane per cell on the f32 layers.  kTable: the host-proved offset table (flags only); else the literal CircleIterator
// walk of the plan kernels' candidate discs (candidate_disc_ok): f64 bounding box, clipped at the map edge, and the f64
// membership test, row-major from the smallest index.
template <bool kTable>
__global__ __launch_bounds__(256) void footmap_direct_kernel(DevMap m, PlanConsts pc, FootmapRoi roi, uint8_t* __restrict__ flags,
                                                             float* __restrict__ height) {
    const size_t idx = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= static_cast<size_t>(roi.nr) * roi.nc) return;
    const int rr = static_cast<int>(idx / static_cast<size_t>(roi.nc));
    const int cc = static_cast<int>(idx - static_cast<size_t>(rr) * roi.nc);
    const int i = roi.row0 + rr, j = roi.col0 + cc;
    float sum = 0.0f, last = 0.0f;
    int cnt = 0;
    bool any = false, failD = false, failC = false, unknown = false;
    auto visit = [&](int qi, int qj) {
        const size_t off = static_cast<size_t>(qi) * m.g.cols + qj;
        const float tv = m.trav[off];
        const bool fin = __builtin_isfinite(tv);
        failD |= fin && tv < pc.thrDefault;    // cpp:2055-2057
        failC |= fin && tv < pc.thrCandidate;  // cpp:2132-2138
        unknown |= !fin;
        any = true;
        if (height) {
            const float e = m.elev[off];
            ordered_step(__builtin_isfinite(e) ? e : 0.0f, sum, last, cnt);  // cpp:2532-2545
        }
    };
    if (kTable) {
        for (int k = 0; k < pc.nFoot; ++k) {
            const int qi = i + pc.footDa[k], qj = j + pc.footDb[k];
            if (in_range(qi, qj, m.g.rows, m.g.cols)) visit(qi, qj);
        }
    } else {
        const double fx = cell_pos(m.g.baseX, m.g.res, i);
        const double fy = cell_pos(m.g.baseY, m.g.res, j);
        const BBox bb = circle_bbox_fast(m.g, fx, fy, pc.rf);
        for (int a = 0; a < bb.ni; ++a)
            for (int b = 0; b < bb.nj; ++b) {
                const int qi = bb.i0 + a, qj = bb.j0 + b;
                if (in_range(qi, qj, m.g.rows, m.g.cols) && cell_in_disc(m.g, qi, qj, fx, fy, pc.rf2)) visit(qi, qj);
            }
    }
    if (flags)
        flags[idx] = static_cast<uint8_t>((any && !failD ? FPE_FMAP_DEFAULT_OK : 0u) | (any && !failC ? FPE_FMAP_CANDIDATE_OK : 0u) |
                                          (unknown ? FPE_FMAP_UNKNOWN : 0u));
    if (height) height[idx] = finish_mean(sum, last, cnt, pc.h);
}

}  // namespace

// Which kernels serve a call with these constants: FPE_E_UNSUPPORTED when the literal walk's box exceeds its bound.
int foothold_map_supported(const PlanConsts& pc, const MapGeom& g) {
    if (pc.footRobust) return pc.footReach <= kHmapMaxReach ? FPE_OK : FPE_E_UNSUPPORTED;
    return std::ceil(pc.rf / g.res) <= kFmapMaxLiteralReach ? FPE_OK : FPE_E_UNSUPPORTED;
}

// bm: the snapshot's planes of (thrDefault, thrCandidate), or words == null when the call has none (then the flags of a proved
// disc with a row-interval form take the table path as well)
hipError_t launch_foothold_map(const DevMap& m, const BitMap& bm, const PlanConsts& pc, const FootmapRoi& roi, uint8_t* d_flags,
                               float* d_height, hipStream_t stream) {
    const size_t n = static_cast<size_t>(roi.nr) * roi.nc;
    const dim3 gridDirect(static_cast<unsigned>((n + 255) / 256));
    if (!pc.footRobust) {
        hipLaunchKernelGGL(footmap_direct_kernel<false>, gridDirect, dim3(256), 0, stream, m, pc, roi, d_flags, d_height);
        return hipGetLastError();
    }
    if (d_flags) {
        if (pc.nHW > 0 && bm.words) {
            const int nWords = ((roi.col0 + roi.nc - 1) >> 5) - (roi.col0 >> 5) + 1;
            const dim3 grid((nWords + kFmapWords - 1) / kFmapWords, (roi.nr + kFmapRows - 1) / kFmapRows);
            hipLaunchKernelGGL(footmap_flags_bits_kernel, grid, dim3(256), 0, stream, bm, m.g.rows, m.g.cols, pc, roi, d_flags);
        } else {
            hipLaunchKernelGGL(footmap_direct_kernel<true>, gridDirect, dim3(256), 0, stream, m, pc, roi, d_flags, static_cast<float*>(nullptr));
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (d_height) {
        const dim3 grid((roi.nc + kHmapCols - 1) / kHmapCols, (roi.nr + kHmapRows - 1) / kHmapRows);
        hipLaunchKernelGGL(footmap_height_kernel, grid, dim3(256), 0, stream, m, pc, roi, d_height);
    }
    return hipGetLastError();
}
