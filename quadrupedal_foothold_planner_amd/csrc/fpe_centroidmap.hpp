// fpe_centroidmap.hpp — part six of the kernel translation unit (included at the end of fpe_kernels.hip, inside
// namespace fpe): the dense centroid map (fpe_centroid_map*, include/fpe.h).
//
// For every cell (i, j) of a region, checkFootholdUseCentroidMethod (cpp:1605-1997) centred on p = getPosition(i, j): what
// centroid_legs_kernel returns for that query, as the code, the offset of the landing cell from (i, j) and z.
//
// The method's geometry is separable by axis (submap_axis, fpe_gridmath.hpp): the rectangle's top-left row i0, its row count ni,
// the submap's x base and the x half of "getSubmap succeeded" depend on the row i only, the y side on the column j only.  So a
// call builds two small tables, one entry per row and one per column of the region (in cmap_rows_kernel), exact for every cell:
// borders, clamped corners and f64 ties included.  The row scan of centroid_scan then splits in two:
//   cmap_rows_kernel   for every map row i' within reach of the region and every column j: cnt = the number of cells of row i'
//                      in the rectangle's columns [j0(j), j0(j) + nj(j)) with trav < defaultFootholdThreshold (the raw `<` of
//                      centroid_scan: NaN is not below, -inf is), from a ballot bit row of the layer in LDS.  Two bits follow:
//                      blocked = cnt > nj * 0.5 (cpp:1743) and below = cnt > 0 (cpp:1649-1658).  Both planes are stored per
//                      column with 32 rows packed into a word, word row k of every column contiguous.  The same kernel
//                      writes the two tables.
//   cmap_code_kernel   one thread per cell: the words of column j over the rows [i0(i), i0(i) + ni(i)) give the whole-region
//                      test (no below bit) and minRow / maxRow (first / last blocked bit, 0 when there is none) with a few
//                      masks and ctz / clz; then the case of centroid_begin, the landing position on the submap and its
//                      getIndex, written as the code and the offset.
//   cmap_z_kernel      z, G lanes per cell as in centroid_legs_kernel: the same scan from the planes, then the plan kernels'
//                      own centre disc (code 0) and centroid_begin / centroid_end.  Nothing about the discs is assumed: z is
//                      what those functions compute, literal_discs or not.
// Every path reads the layer itself, so maps without bit planes need nothing else.  The only bound is the reach H of the
// rectangle (ceil(R / res) + 2 rows or columns from the cell): at most kCmapMaxReach, which keeps every offset in int8;
// larger radii are FPE_E_UNSUPPORTED (centroid_legs_kernel has no such bound).
#pragma once

constexpr int kCmapMaxReach = 100;  // |landing - cell| <= H <= 100 fits the int8 offsets

namespace {

constexpr int kCmapCols = 256;                                               // columns per code workgroup
constexpr int kCmapRowCols = 64;                                             // columns per plane workgroup
constexpr int kCmapSpanWords = (kCmapRowCols + 2 * kCmapMaxReach + 63) / 64;  // 64-bit words of a plane row in LDS

// The scan of centroid_scan for cell (i, j) from the planes: a = first row of the rectangle relative to the planes' rb
__device__ __forceinline__ CentroidScan cmap_scan(const SubmapAxis& ra, const SubmapAxis& ca, const uint32_t* __restrict__ blocked,
                                                  const uint32_t* __restrict__ below, int nc, int c, int a, int nwr) {
    CentroidScan sc;
    bool anyBelow = false;
    int first = -1, last = -1;
    const int e = a + ra.ni;  // rows [a, e)
    for (int k = a >> 5; k <= (e - 1) >> 5; ++k) {
        const int lo = max(a - 32 * k, 0), hi = min(e - 32 * k, 32);
        const uint32_t m = (hi - lo == 32 ? 0xFFFFFFFFu : ((1u << (hi - lo)) - 1u)) << lo;
        const size_t w = static_cast<size_t>(min(max(k, 0), nwr - 1)) * nc + c;  // k is inside the planes by the reach bound
        const uint32_t bl = blocked[w] & m;
        anyBelow |= (below[w] & m) != 0u;
        if (bl != 0u) {
            if (first < 0) first = 32 * k + __builtin_ctz(bl) - a;
            last = 32 * k + 31 - __builtin_clz(bl) - a;
        }
    }
    sc.whole = ra.ni * ca.ni > 0 && !anyBelow;
    sc.minRow = first < 0 ? 0 : first;  // no blocked row: as if row 0 were
    sc.maxRow = last < 0 ? 0 : last;
    return sc;
}

// The case of centroid_begin (cpp:1777-1952) once the region is not wholly valid: the code 1-4 with the submap indices of the
// result, or 5 (first and last row blocked: no branch taken)
__device__ __forceinline__ int cmap_case(const CentroidScan& sc, int ni, int nj, int& newRow, int& newCol) {
    const int bottomRow = ni - 1, rightCol = nj - 1;
    const int minRow = sc.minRow, maxRow = sc.maxRow;
    if (minRow == 0 && maxRow != bottomRow) {  // case 1, cpp:1777-1786
        newRow = static_cast<int>(floor((maxRow + bottomRow + 1) * 0.5));
        newCol = static_cast<int>(floor((rightCol + 1) * 0.5));
        return 1;
    }
    if (minRow != 0 && maxRow != bottomRow) {  // case 2, cpp:1843-1886
        newCol = static_cast<int>(floor((rightCol + 0) * 0.5));
        if ((minRow - 0) >= (bottomRow - maxRow)) {
            newRow = static_cast<int>(ceil(minRow * 0.5));
            return 2;
        }
        newRow = static_cast<int>(floor((maxRow + bottomRow) * 0.5));
        return 3;
    }
    if (minRow != 0 && maxRow == bottomRow) {  // case 3, cpp:1944-1952
        newRow = static_cast<int>(ceil(minRow * 0.5));
        newCol = static_cast<int>(floor((rightCol + 0) * 0.5));
        return 4;
    }
    newRow = newCol = 0;
    return 5;
}

// Word row k = blockIdx.y of the blocked / below planes for kCmapRowCols columns of the region, and the per-axis tables: the
// block's own column entries (every block, in LDS; the blocks of word row 0 also store them), and with blockIdx.x == 0 the
// region's rows 32 k .. 32 k + 31 (nwr * 32 >= nr: the planes cover the region's rows).  Thread t: column t & 63, rows
// 8 (t >> 6) .. 8 (t >> 6) + 7 of the word.
__global__ __launch_bounds__(256) void cmap_rows_kernel(DevMap m, PlanConsts pc, CmapConsts cc, FootmapRoi roi,
                                                        SubmapAxis* __restrict__ rowTab, SubmapAxis* __restrict__ colTab,
                                                        uint32_t* __restrict__ blocked, uint32_t* __restrict__ below) {
    __shared__ unsigned long long sRow[32 * kCmapSpanWords];  // bit b of word w of row rr: trav(ib + rr, cbase + 64 w + b) below
    __shared__ SubmapAxis sCol[kCmapRowCols];
    __shared__ uint32_t sBits[2][4][kCmapRowCols];
    const MapGeom& g = m.g;
    const int t = static_cast<int>(threadIdx.x), lane = t & 63, wv = t >> 6;
    const int jb = roi.col0 + static_cast<int>(blockIdx.x) * kCmapRowCols;
    const int cbase = max(jb - cc.H, 0);
    const int nW = min((kCmapRowCols + 2 * cc.H + 63) >> 6, kCmapSpanWords);  // H <= kCmapMaxReach (host): the clamp never acts
    const int k = static_cast<int>(blockIdx.y), ib = cc.rb + 32 * k;
    const int cols = g.cols, total = 32 * nW;
    if (t < kCmapRowCols && jb + t < roi.col0 + roi.nc) {
        const SubmapAxis a = submap_axis(g.orgY, g.posY, g.lenY, g.baseY, g.res, g.rinv, g.cols, cell_pos(g.baseY, g.res, jb + t),
                                         static_cast<double>(cc.Rf));
        sCol[t] = a;
        if (k == 0) colTab[jb - roi.col0 + t] = a;
    } else if (t >= 64 && t < 96 && blockIdx.x == 0 && 32 * k + (t - 64) < roi.nr) {
        const int r = 32 * k + (t - 64);
        rowTab[r] = submap_axis(g.orgX, g.posX, g.lenX, g.baseX, g.res, g.rinv, g.rows, cell_pos(g.baseX, g.res, roi.row0 + r),
                                static_cast<double>(cc.Rf * 2));
    }
    for (int e0 = wv; e0 < total; e0 += 16) {  // four independent loads per lane, then their ballots
        bool b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 4 * u, rr = e / nW, wd = e - rr * nW;
            const int i = ib + rr, col = cbase + 64 * wd + lane;
            b[u] = e < total && i < cc.re && col < cols && m.trav[static_cast<size_t>(i) * cols + col] < pc.thrDefault;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 4 * u;
            const unsigned long long mask = __ballot(b[u]);
            if (lane == 0 && e < total) sRow[(e / nW) * kCmapSpanWords + (e % nW)] = mask;
        }
    }
    __syncthreads();
    const int c = jb - roi.col0 + lane;
    uint32_t bl = 0u, bw = 0u;
    if (c < roi.nc && sCol[lane].ok != 0) {
        const SubmapAxis ca = sCol[lane];
        const int nj = ca.ni, rightCol = nj - 1;
        const int s = min(max(ca.i0 - cbase, 0), 64 * nW), e = min(s + nj, 64 * nW);  // inside the row by the reach bound
        for (int rr = 8 * wv; rr < 8 * wv + 8 && ib + rr < cc.re; ++rr) {
            const unsigned long long* row = sRow + rr * kCmapSpanWords;
            int cnt = 0;
            for (int x = s; x < e;) {
                const int wd = x >> 6, o = x & 63, take = min(64 - o, e - x);
                unsigned long long v = row[wd] >> o;
                if (take < 64) v &= (1ull << take) - 1ull;
                cnt += __builtin_popcountll(v);
                x += take;
            }
            if (cnt > ((rightCol + 1) * 0.5)) bl |= 1u << rr;  // cpp:1743
            if (cnt > 0) bw |= 1u << rr;
        }
    }
    sBits[0][wv][lane] = bl;
    sBits[1][wv][lane] = bw;
    __syncthreads();
    if (t < kCmapRowCols && c < roi.nc) {
        const size_t w = static_cast<size_t>(k) * roi.nc + c;
        blocked[w] = sBits[0][0][t] | sBits[0][1][t] | sBits[0][2][t] | sBits[0][3][t];
        below[w] = sBits[1][0][t] | sBits[1][1][t] | sBits[1][2][t] | sBits[1][3][t];
    }
}

// Code and offset of every cell of the region
__global__ __launch_bounds__(256) void cmap_code_kernel(MapGeom g, CmapConsts cc, FootmapRoi roi, const SubmapAxis* __restrict__ rowTab,
                                                        const SubmapAxis* __restrict__ colTab, const uint32_t* __restrict__ blocked,
                                                        const uint32_t* __restrict__ below, uint8_t* __restrict__ code,
                                                        int8_t* __restrict__ offset) {
    const int c = static_cast<int>(blockIdx.x) * kCmapCols + static_cast<int>(threadIdx.x);
    const int r = static_cast<int>(blockIdx.y);
    if (c >= roi.nc) return;
    const int i = roi.row0 + r, j = roi.col0 + c;
    const SubmapAxis ra = rowTab[r], ca = colTab[c];
    int cd = 6, di = 0, dj = 0;
    if (ra.ok != 0 && ca.ok != 0) {
        const CentroidScan sc = cmap_scan(ra, ca, blocked, below, roi.nc, c, ra.i0 - cc.rb, cc.nwr);
        if (sc.whole) {
            cd = 0;
        } else {
            int newRow, newCol;
            cd = cmap_case(sc, ra.ni, ca.ni, newRow, newCol);
            if (cd != 5) {  // getIndex of the submap's getPosition (cpp:1816)
                di = index_of_fast(cell_pos(ra.base, g.res, newRow), g.orgX, g.posX, g.res, g.rinv) - i;
                dj = index_of_fast(cell_pos(ca.base, g.res, newCol), g.orgY, g.posY, g.res, g.rinv) - j;
            }
        }
    }
    const size_t idx = static_cast<size_t>(r) * roi.nc + c;
    if (code) code[idx] = static_cast<uint8_t>(cd);
    if (offset) {
        offset[2 * idx] = static_cast<int8_t>(di);
        offset[2 * idx + 1] = static_cast<int8_t>(dj);
    }
}

// z of every cell of the region: G lanes per cell, the ordered-sum scratch in the group's LDS tile (centroid_legs_kernel)
template <int G, bool kMid = false>
__global__ __launch_bounds__(256) void cmap_z_kernel(DevMap m, PlanConsts pc, CmapConsts cc, FootmapRoi roi,
                                                     const SubmapAxis* __restrict__ rowTab, const SubmapAxis* __restrict__ colTab,
                                                     const uint32_t* __restrict__ blocked, const uint32_t* __restrict__ below,
                                                     float* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = static_cast<int>(threadIdx.x);
    const int w = tid / G;
    const Grp<G> g(tid);
    const long long q = static_cast<long long>(blockIdx.x) * (256 / G) + w;
    float* scratch = reinterpret_cast<float*>(smem + static_cast<size_t>(w) * tile_total_bytes(pc));
    if (q >= static_cast<long long>(roi.nr) * roi.nc) return;
    const int r = static_cast<int>(q / roi.nc), c = static_cast<int>(q - static_cast<long long>(r) * roi.nc);
    const SubmapAxis ra = rowTab[r], ca = colTab[c];
    Submap s;
    s.ok = ra.ok != 0 && ca.ok != 0;
    s.i0 = ra.i0;
    s.ni = ra.ni;
    s.baseX = ra.base;
    s.j0 = ca.i0;
    s.nj = ca.ni;
    s.baseY = ca.base;
    LegCtx lc;
    lc.cx = cell_pos(m.g.baseX, m.g.res, roi.row0 + r);  // getPosition(i, j)
    lc.cy = cell_pos(m.g.baseY, m.g.res, roi.col0 + c);
    lc.ici = lc.icj = -1;
    CentroidScan sc;
    sc.whole = false;
    sc.minRow = sc.maxRow = 0;
    if (s.ok) sc = cmap_scan(ra, ca, blocked, below, roi.nc, c, ra.i0 - cc.rb, cc.nwr);
    float zCentre = 0.0f;
    if (sc.whole) {  // as centroid_legs_kernel
        const Box b0{lc.cx, lc.cy, pc.rf, pc.rf};
        Corners<G, 8> cs;
        cs.eval(m.g, g, b0, b0, b0, b0, 0x2u);
        const BBox bb = cs.template bbox<0>(g);
        lc.ici = cs.template get<4>(g);
        lc.icj = cs.template get<5>(g);
        DiscLoads dc;
        disc_issue<G, true, kMid>(m, pc, lc.cx, lc.cy, bb, g, dc);
        bool unused;
        zCentre = disc_consume<G, true, kMid>(m, pc, lc.cx, lc.cy, bb, g, dc, unused, scratch);
    }
    CentroidPending cp;
    centroid_begin<G, kMid>(m, pc, lc, s, sc, zCentre, g, cp);
    centroid_end<G, kMid>(m, pc, g, cp, scratch);
    if (g.sub == 0) z[q] = cp.o.z;
}

}  // namespace

// The constants of a dense call for search radius R over `roi`; false when the rectangle's reach is over kCmapMaxReach
bool centroid_map_consts(const MapGeom& g, const FootmapRoi& roi, float R, CmapConsts& cc) {
    cc.Rf = R;
    const double reach = std::ceil(static_cast<double>(R) / g.res) + 2.0;
    if (!(reach <= kCmapMaxReach)) return false;
    cc.H = static_cast<int32_t>(reach);
    cc.rb = std::max(roi.row0 - cc.H, 0);
    cc.re = std::min(roi.row0 + roi.nr + cc.H, g.rows);
    cc.nwr = (cc.re - cc.rb + 31) / 32;
    return true;
}

// Scratch of a dense call: the two tables, then the two planes
size_t centroid_map_scratch_bytes(const FootmapRoi& roi, const CmapConsts& cc) {
    const size_t tabs = (static_cast<size_t>(roi.nr) + roi.nc) * sizeof(SubmapAxis);
    return ((tabs + 255) & ~static_cast<size_t>(255)) + 2 * static_cast<size_t>(cc.nwr) * roi.nc * sizeof(uint32_t);
}

hipError_t launch_centroid_map(const DevMap& m, const PlanConsts& pc, const CmapConsts& cc, const FootmapRoi& roi, void* scratch,
                               uint8_t* d_code, int8_t* d_offset, float* d_z, hipStream_t stream) {
    SubmapAxis* rowTab = static_cast<SubmapAxis*>(scratch);
    SubmapAxis* colTab = rowTab + roi.nr;
    const size_t tabs = (static_cast<size_t>(roi.nr) + roi.nc) * sizeof(SubmapAxis);
    uint32_t* blocked = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(scratch) + ((tabs + 255) & ~static_cast<size_t>(255)));
    uint32_t* below = blocked + static_cast<size_t>(cc.nwr) * roi.nc;
    hipLaunchKernelGGL(cmap_rows_kernel, dim3((roi.nc + kCmapRowCols - 1) / kCmapRowCols, cc.nwr), dim3(256), 0, stream, m, pc, cc, roi,
                       rowTab, colTab, blocked, below);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int colBlocks = (roi.nc + kCmapCols - 1) / kCmapCols;
    if (d_code || d_offset) {
        hipLaunchKernelGGL(cmap_code_kernel, dim3(colBlocks, roi.nr), dim3(256), 0, stream, m.g, cc, roi, rowTab, colTab, blocked, below,
                           d_code, d_offset);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (d_z) {
        const long long n = static_cast<long long>(roi.nr) * roi.nc;
        const size_t lds = centroid_lds_bytes(pc);
        if (search_group_size(pc) == 8 && mid_variant(pc, m.g.res))
            hipLaunchKernelGGL((cmap_z_kernel<8, true>), dim3(static_cast<unsigned>((n + 31) / 32)), dim3(256), lds, stream, m, pc, cc, roi,
                               rowTab, colTab, blocked, below, d_z);
        else if (search_group_size(pc) == 8)
            hipLaunchKernelGGL(cmap_z_kernel<8>, dim3(static_cast<unsigned>((n + 31) / 32)), dim3(256), lds, stream, m, pc, cc, roi, rowTab,
                               colTab, blocked, below, d_z);
        else
            hipLaunchKernelGGL(cmap_z_kernel<64>, dim3(static_cast<unsigned>((n + 3) / 4)), dim3(256), lds, stream, m, pc, cc, roi, rowTab,
                               colTab, blocked, below, d_z);
        e = hipGetLastError();
    }
    return e;
}

hipError_t set_max_lds_centroid_map(size_t bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cmap_z_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(bytes));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(cmap_z_kernel<8, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(bytes));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(cmap_z_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(bytes));
}
