// fpe_footsnap.hpp — part five of the kernel translation unit (included at the end of fpe_kernels.hip, inside
// namespace fpe): the dense snap map (fpe_foothold_snap*, include/fpe.h).
//
// For every cell (i, j) of a region, checkFoothold (cpp:2001-2036) at the cell centre p = getPosition(i, j) with the search
// polygon getSearchPolygon(p, R) (or the plan kernels' hexagon): where the planner puts a foot aimed at the cell.  Output =
// what fpe_search_legs returns for that query, as a landing offset (di, dj), a source byte and the mean height z.
//
// Two paths, chosen on the host (prepare_foothold_snap / run_foothold_snap in fpe_engine.cpp):
//   footsnap_bits_kernel   the proved path.  The default hits are the Df dilation of the foothold-map flag kernel.  The
//                          spiral search of every other cell is a "first-hit dilation" over 32-cell words: the candidate-pass
//                          plane P = in-map & ~dilate(C, disc) of the tile plus a halo of nRings sits in LDS; a wavefront walks
//                          the spiral rank table in order and ANDs the shifted P word of each offset into its lanes'
//                          not-yet-found masks, recording the offset of every new hit, until a ballot says all its cells are
//                          resolved.  The reference rectangle becomes index bounds |di| <= rectA, |dj| <= rectB, and the ring
//                          filter of the outer two rings (SpiralIterator::generateRing's isInside) an integer bound on
//                          di^2 + dj^2, both proved translation-invariant by the host for this map and radius
//                          (snap_prove).  A candidate whose foot disc crosses the rectangle's edge is also valid only when
//                          every disc cell outside it is non-finite (cpp:2132-2138): an AND of shifted ~F words.  z comes
//                          from footmap_height_kernel, set to 0 here where the search found nothing.
//   the literal path       everything the proof does not cover (the hexagon, rectangle or ring-filter ties within rounding,
//                          discs without the bit-plane form, literal_discs, more than kSnapMaxRings rings): the cells' queries
//                          are built on the device in chunks and run through search_legs_kernel itself, then converted.
#pragma once

// The bit path holds P for a halo of nRings rows and one word per side: rings up to 32
constexpr int kSnapMaxRings = 32;
// Cells per literal-path chunk (queries + records of a chunk live in stream-ordered scratch)
constexpr int kSnapChunk = 1 << 18;

namespace {

constexpr int kSnapRows = 8;                                  // rows per workgroup (one tiled line)
constexpr int kSnapWords = 32;                                // words per workgroup (1024 columns)
constexpr int kSnapPWords = kSnapWords + 3;                   // P: words w0-1 .. w0+33
constexpr int kSnapCWords = kSnapWords + 5;                   // C, ~F: words w0-2 .. w0+34
constexpr int kSnapPRows = kSnapRows + 2 * kSnapMaxRings;     // P: rows i0-H .. i0+7+H
constexpr int kSnapCRows = kSnapPRows + 2 * kHmapMaxReach;    // C, ~F: rows i0-H-R .. i0+7+H+R

// 32 bits of a plane row starting at column 32 w + s (w = w0 + wl; s may be negative), from the LDS words of that row: `bias`
// = the words the array holds left of w0 (1 for P, 2 for ~F)
__device__ __forceinline__ uint32_t snap_shifted(const uint32_t* row, int wl, int s, int bias) {
    const int q = wl + bias + (s >> 5), o = s & 31;
    const uint64_t v = (static_cast<uint64_t>(row[q + 1]) << 32) | row[q];
    return static_cast<uint32_t>(v >> o);
}

__global__ __launch_bounds__(256) void footsnap_bits_kernel(BitMap bm, int rows, int cols, PlanConsts pc, SnapConsts sc,
                                                            SpiralLut lut, FootmapRoi roi, int8_t* __restrict__ offset,
                                                            uint8_t* __restrict__ source, float* __restrict__ z) {
    __shared__ uint32_t sC[kSnapCRows * kSnapCWords];   // C plane
    __shared__ uint32_t sNF[kSnapCRows * kSnapCWords];  // ~F (non-finite or outside the map)
    __shared__ uint32_t sP[kSnapPRows * kSnapPWords];   // candidate-pass plane P
    __shared__ uint8_t sSrc[kSnapRows * kSnapWords * 32];
    __shared__ uint16_t sOff[kSnapRows * kSnapWords * 32];
    const int t = static_cast<int>(threadIdx.x);
    const int r = t & 7, wl = t >> 3;
    const int w0 = (roi.col0 >> 5) + static_cast<int>(blockIdx.x) * kSnapWords;
    const int i0 = roi.row0 + static_cast<int>(blockIdx.y) * kSnapRows;
    const int w = w0 + wl, i = i0 + r;
    const int lastI = roi.row0 + roi.nr - 1, colEnd = roi.col0 + roi.nc;
    const int R = pc.footReach, H = sc.nRings;
    // ---- default hits: the Df dilation (footmap_flags_bits_kernel) ----
    uint32_t notFound = 0u;
    if (i <= lastI) {
        uint32_t dDf = 0u;
        for (int a = -R; a <= R; ++a) {
            const int q = min(max(i + a, -1), rows);
            const uint4 gp = bm.words[bit_group_index(q, min(w - 1, bm.nw), bm.strideW)];
            const uint4 gc = bm.words[bit_group_index(q, min(w, bm.nw), bm.strideW)];
            const uint4 gn = bm.words[bit_group_index(q, min(w + 1, bm.nw), bm.strideW)];
            dDf |= fmap_hdilate(gp.y, gc.y, gn.y, pc.hwList[pc.hwIdx[a < 0 ? -a : a]]);
        }
        // cells of the region in this word
        const int lo = max(roi.col0 - 32 * w, 0), hi = min(colEnd - 32 * w, 32);
        const uint32_t inRoi = hi <= lo ? 0u : ((hi - lo == 32 ? 0xFFFFFFFFu : ((1u << (hi - lo)) - 1u)) << lo);
        notFound = dDf & inRoi;
    }
    for (int b = 0; b < 32; ++b) {
        sSrc[r * 1024 + wl * 32 + b] = static_cast<uint8_t>((notFound >> b) & 1u) * 2u;
        sOff[r * 1024 + wl * 32 + b] = 0;
    }
    if (__syncthreads_or(notFound != 0u)) {
        // ---- C and ~F of the haloed tile, then P ----
        const int cRows = kSnapRows + 2 * (H + R), pRows = kSnapRows + 2 * H;
        for (int k = t; k < cRows * kSnapCWords; k += 256) {
            const int a = k / kSnapCWords, b = k - a * kSnapCWords;
            const int q = min(max(i0 - H - R + a, -1), rows);
            const int ww = min(max(w0 - 2 + b, -1), bm.nw);
            const uint4 g = bm.words[bit_group_index(q, ww, bm.strideW)];
            sC[a * kSnapCWords + b] = g.z;
            sNF[a * kSnapCWords + b] = ~g.w;  // F is zero outside the map
        }
        __syncthreads();
        for (int k = t; k < pRows * kSnapPWords; k += 256) {
            const int a = k / kSnapPWords, b = k - a * kSnapPWords;  // P row i0 - H + a, word w0 - 1 + b
            const int q = i0 - H + a;
            uint32_t d = 0u;
            for (int e = -R; e <= R; ++e) {
                const uint32_t* cr = sC + (a + R + e) * kSnapCWords + b;  // C words w0-2+b .. w0+b
                d |= fmap_hdilate(cr[0], cr[1], cr[2], pc.hwList[pc.hwIdx[e < 0 ? -e : e]]);
            }
            const uint32_t inMap = (q >= 0 && q < rows) ? fmap_col_mask(w0 - 1 + b, cols) : 0u;
            sP[a * kSnapPWords + b] = ~d & inMap;
        }
        __syncthreads();
        // ---- first-hit dilation in spiral rank order, wave-uniform offsets ----
        const uint32_t* pRow = sP + (r + H) * kSnapPWords;  // P row of this lane's row at di = 0
        const uint32_t* fRow = sNF + (r + H + R) * kSnapCWords;
        for (int k = 0; k < sc.nCand; ++k) {
            if (__ballot(notFound != 0u) == 0ull) break;
            const int di = lut.di[k], dj = lut.dj[k], ring = lut.ring[k];
            if (ring >= 1 && (ring == sc.nRings || ring + 1 == sc.nRings) && di * di + dj * dj > sc.ringT) continue;
            uint32_t hit = notFound & snap_shifted(pRow + di * kSnapPWords, wl, dj, 1);
            const int adi = di < 0 ? -di : di, adj = dj < 0 ? -dj : dj;
            if (hit != 0u && (adi + R > sc.rectA || adj + R > sc.rectB)) {
                // the disc crosses the rectangle's edge: its cells outside must be non-finite (or outside the map)
                for (int e = 0; e < pc.nFoot && hit != 0u; ++e) {
                    const int qa = di + pc.footDa[e], qb = dj + pc.footDb[e];
                    if ((qa < 0 ? -qa : qa) > sc.rectA || (qb < 0 ? -qb : qb) > sc.rectB)
                        hit &= snap_shifted(fRow + qa * kSnapCWords, wl, qb, 2);
                }
            }
            notFound &= ~hit;
            const uint16_t packed = static_cast<uint16_t>((static_cast<uint32_t>(di) & 0xFFu) | ((static_cast<uint32_t>(dj) & 0xFFu) << 8));
            while (hit != 0u) {
                const int b = __builtin_ctz(hit);
                hit &= hit - 1u;
                sSrc[r * 1024 + wl * 32 + b] = 1u;
                sOff[r * 1024 + wl * 32 + b] = packed;
            }
        }
    }
    __syncthreads();
    const int colBase = 32 * w0;
    for (int k = t; k < kSnapRows * kSnapWords * 32; k += 256) {
        const int rr = k >> 10, cc = k & 1023;
        const int ii = i0 + rr, jj = colBase + cc;
        if (ii <= lastI && jj >= roi.col0 && jj < colEnd) {
            const size_t idx = static_cast<size_t>(ii - roi.row0) * roi.nc + (jj - roi.col0);
            const uint8_t s = sSrc[k];
            if (source) source[idx] = s;
            if (offset) {
                const uint16_t o = sOff[k];
                offset[2 * idx] = static_cast<int8_t>(o & 0xFFu);
                offset[2 * idx + 1] = static_cast<int8_t>(o >> 8);
            }
            if (z && s == 2) z[idx] = 0.0f;
        }
    }
}

// The literal path, one chunk of cells [c0, c0 + n) of the region: the queries of the contract (include/fpe.h) ...
__global__ __launch_bounds__(256) void footsnap_queries_kernel(MapGeom g, SnapConsts sc, FootmapRoi roi, long long c0, int n,
                                                               fpe_leg_query* __restrict__ q) {
    const int k = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (k >= n) return;
    const long long c = c0 + k;
    const int i = roi.row0 + static_cast<int>(c / roi.nc), j = roi.col0 + static_cast<int>(c % roi.nc);
    fpe_leg_query o;
    o.cx = cell_pos(g.baseX, g.res, i);  // getPosition(i, j)
    o.cy = cell_pos(g.baseY, g.res, j);
    o.search_radius = sc.Rf;
    const double rr = static_cast<double>(sc.Rf);
    for (int v = 0; v < FPE_MAX_POLYGON_VERTICES; ++v) o.vx[v] = o.vy[v] = 0.0;
    if (sc.polyKind == 0) {  // getSearchPolygon (cpp:2496-2517): LU, RU, RD, LD
        o.n_vertices = 4;
        o.vx[0] = o.cx + rr;  o.vy[0] = o.cy + 0.5 * rr;
        o.vx[1] = o.cx + rr;  o.vy[1] = o.cy - 0.5 * rr;
        o.vx[2] = o.cx - rr;  o.vy[2] = o.cy - 0.5 * rr;
        o.vx[3] = o.cx - rr;  o.vy[3] = o.cy + 0.5 * rr;
    } else {  // the plan kernels' hexagon (leg_phase)
        const double hx = 0.5 * rr;
        const double hy = (0.5 * rr) * 0.8660254037844386;
        o.n_vertices = 6;
        o.vx[0] = o.cx + rr;  o.vy[0] = o.cy;
        o.vx[1] = o.cx + hx;  o.vy[1] = o.cy - hy;
        o.vx[2] = o.cx - hx;  o.vy[2] = o.cy - hy;
        o.vx[3] = o.cx - rr;  o.vy[3] = o.cy;
        o.vx[4] = o.cx - hx;  o.vy[4] = o.cy + hy;
        o.vx[5] = o.cx + hx;  o.vy[5] = o.cy + hy;
    }
    q[k] = o;
}

// ... and their search_legs_kernel records as snap products
__global__ __launch_bounds__(256) void footsnap_convert_kernel(FootmapRoi roi, long long c0, int n, const fpe_foothold* __restrict__ f,
                                                               int8_t* __restrict__ offset, uint8_t* __restrict__ source,
                                                               float* __restrict__ z) {
    const int k = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (k >= n) return;
    const long long c = c0 + k;
    const int i = roi.row0 + static_cast<int>(c / roi.nc), j = roi.col0 + static_cast<int>(c % roi.nc);
    const fpe_foothold o = f[k];
    const bool spiral = o.source == 1;
    if (source) source[c] = o.source;
    if (offset) {
        offset[2 * c] = static_cast<int8_t>(spiral ? o.row - i : 0);
        offset[2 * c + 1] = static_cast<int8_t>(spiral ? o.col - j : 0);
    }
    if (z) z[c] = o.z;
}

}  // namespace

// Proved path: pc.footRobust with a row-interval form, the planes, a rectangle the host proved, rings within the halo
bool foothold_snap_bits_ok(const PlanConsts& pc, const SnapConsts& sc, bool haveBits, bool rectProved) {
    return haveBits && pc.footRobust && pc.nHW > 0 && pc.footReach <= kHmapMaxReach && sc.polyKind == 0 && rectProved &&
           sc.nRings <= kSnapMaxRings;
}

hipError_t launch_foothold_snap_bits(const DevMap& m, const BitMap& bm, const PlanConsts& pc, const SnapConsts& sc, const SpiralLut& lut,
                                     const FootmapRoi& roi, int8_t* d_offset, uint8_t* d_source, float* d_z, hipStream_t stream) {
    if (d_z) {  // the ordered sums of the foothold map; the snap kernel then zeroes the cells without a foothold
        const hipError_t e = launch_foothold_map(m, bm, pc, roi, nullptr, d_z, stream);
        if (e != hipSuccess) return e;
    }
    const int nWords = ((roi.col0 + roi.nc - 1) >> 5) - (roi.col0 >> 5) + 1;
    const dim3 grid((nWords + kSnapWords - 1) / kSnapWords, (roi.nr + kSnapRows - 1) / kSnapRows);
    hipLaunchKernelGGL(footsnap_bits_kernel, grid, dim3(256), 0, stream, bm, m.g.rows, m.g.cols, pc, sc, lut, roi, d_offset, d_source, d_z);
    return hipGetLastError();
}

// The literal path's scratch: kSnapChunk queries, then kSnapChunk records
size_t foothold_snap_literal_scratch_bytes() {
    return static_cast<size_t>(kSnapChunk) * (sizeof(fpe_leg_query) + sizeof(fpe_foothold));
}

hipError_t launch_foothold_snap_literal(const DevMap& m, const PlanConsts& pc, const SnapConsts& sc, const SpiralLut& lut,
                                        const FootmapRoi& roi, void* scratch, int8_t* d_offset, uint8_t* d_source, float* d_z,
                                        hipStream_t stream) {
    fpe_leg_query* q = static_cast<fpe_leg_query*>(scratch);
    fpe_foothold* f = reinterpret_cast<fpe_foothold*>(static_cast<unsigned char*>(scratch) + static_cast<size_t>(kSnapChunk) * sizeof(fpe_leg_query));
    const long long total = static_cast<long long>(roi.nr) * roi.nc;
    for (long long c0 = 0; c0 < total; c0 += kSnapChunk) {
        const int n = static_cast<int>(std::min<long long>(kSnapChunk, total - c0));
        const dim3 grid((n + 255) / 256);
        hipLaunchKernelGGL(footsnap_queries_kernel, grid, dim3(256), 0, stream, m.g, sc, roi, c0, n, q);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_search_legs(m, pc, lut, q, n, f, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(footsnap_convert_kernel, grid, dim3(256), 0, stream, roi, c0, n, f, d_offset, d_source, d_z);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
