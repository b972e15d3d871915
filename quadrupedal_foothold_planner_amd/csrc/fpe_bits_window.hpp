// fpe_bits_window.hpp — the bit-window kernels, first piece (included by fpe_bits.hpp, inside namespace fpe; not stand-alone):
// what BOTH kernel families are made of.  The bit-plane build, the window rows and a leg's row arrays in LDS, the y entry,
// the lane exchanges and row shifts, the window loads, the centroid row scan and case logic, the default check, the search
// polygon as row / column intervals, the erosion and the candidate scan (spiral_bits), and the side-by-side mean heights
// that flush_seqrec2 (fpe_bits_seq.hpp) and flush_unit_g (fpe_bits_lane8.hpp) share.
#pragma once

namespace {

// ---- bit-plane build: one wavefront ballots 64 columns of a row ---------------------------------------------
__global__ __launch_bounds__(256) void build_bitmap_kernel(const float* __restrict__ trav, int rows, int cols, float thrD,
                                                           float thrC, uint4* __restrict__ words, int strideW, int nw) {
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
    const bool in = j < cols;
    float v = 0.0f;
    if (in) v = trav[static_cast<size_t>(i) * cols + j];
    const bool fin = in && __builtin_isfinite(v);
    const bool d = in && v < thrD;  // raw compare: NaN -> false, -inf -> true (cpp:1653, 1736)
    const bool c = fin && v < thrC;
    const unsigned long long bD = __ballot(d), bDf = __ballot(d && fin), bC = __ballot(c), bF = __ballot(fin);
    const int lane = static_cast<int>(threadIdx.x) & 63;
    if (lane < 2) {
        const int w = (blockIdx.x * 256 + (static_cast<int>(threadIdx.x) & ~63)) / 32 + lane;
        if (w < nw) {
            uint4 o;
            o.x = static_cast<unsigned>(bD >> (32 * lane));
            o.y = static_cast<unsigned>(bDf >> (32 * lane));
            o.z = static_cast<unsigned>(bC >> (32 * lane));
            o.w = static_cast<unsigned>(bF >> (32 * lane));
            words[bit_group_index(i, w, strideW)] = o;
        }
    }
}

// (bit_group_index: fpe_device.hpp — the tiled plane layout, shared with win_issue)

// Synchronisation of the lanes of a pose in the bit-window kernels.  A pose never spans more than ONE wavefront here
// (8 lanes per leg: half a wavefront; one wavefront per pose), and the LDS operations of a wavefront execute in order:
// the compiler must not reorder across the point, nothing has to be waited for.  (pose_sync<64> of the direct kernels is
// a workgroup barrier — a pose owns four wavefronts there — which also waits for every outstanding global load and
// store of the wavefront: in the one-wavefront-per-pose kernels that serialised the leg's loads with its LDS hand-offs.)
template <int G>
__device__ __forceinline__ void bits_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// 64-lane kernels: upper bound of a CircleIterator bounding box (cells): two rounds of 64 membership tests
constexpr int kBitsMaxBoxCells = 128;

// ---- window rows ------------------------------------------------------------------------------------------
// A window row is KW 32-bit words per plane (KW = 1: windows of up to 32 columns, the 8-lane kernels; 2 / 3: the
// one-wavefront-per-pose kernels of 1 cm / 0.5 cm maps).
template <int NRL, int KW>
struct WinRows {
    uint32_t D[NRL][KW], Df[NRL][KW], C[NRL][KW], F[NRL][KW];
};
// Per-leg LDS: row masks shared between the lanes of the leg's group — a: Df rows, later P rows, then E rows (row-
// interval erosion); f: F rows for polygons that are not folded into P; h[k]: single-word rows: horizontally eroded P rows,
// one array per distinct row half-width of the disc; multi-word rows: ONE array, the E rows of the nested erosion (h[0]
// is also the E rows of the offset-by-offset erosion, and f / h[0] the scratch of the polygon's row masks).  Arrays hold `rows` window rows of KW words (the 64-lane kernels allocate 2 winH + 1 rows, not 64 * NRL:
// LDS, not registers, bounds their occupancy).  The row arrays double as float scratch of a direct disc pass.
struct LegBits {
    uint32_t* a;
    uint32_t* f;
    uint32_t* h0;  // array k of the eroded rows at h0 + k * hStride (a pointer array indexed at run time would live in scratch)
    int hStride;
    int rows;
};
// words (4 bytes) of one leg's LDS: the row arrays
__host__ __device__ __forceinline__ int legbits_words(int rows, int kw, int nHW) {
    // (multi-word rows use three of the arrays only since the nested erosion; the others stay: shrinking the allocation
    // to three arrays was measured 1.5 % SLOWER on cfg-3, neutral on cfg-5 — kept as measured)
    const int arrays = 2 + (nHW > 0 ? nHW : 1);
    return (arrays * rows * kw + 3) & ~3;
}
__device__ __forceinline__ LegBits make_legbits(unsigned char* base, int rows, int kw) {
    LegBits lb;
    uint32_t* p = reinterpret_cast<uint32_t*>(base);
    const int n = rows * kw;
    lb.rows = rows;
    lb.a = p;
    lb.f = p + n;
    lb.h0 = p + 2 * n;
    lb.hStride = n;
    return lb;
}

// The y side of a leg's geometry for one gait cycle (8-lane kernels; see fill_yentry, fpe_bits_lane8.hpp).
struct YEntry {
    int jc;        // getIndex(centre), column
    int j0d, njd;  // foot-disc box columns (centre disc and default-track disc: same y, same radius)
    int j0r, njr;  // centroid rectangle columns (getSubmap, cpp:1615-1627)
    int jA, jB;    // reference rectangle polygon: the columns j with ylo <= y_j < yhi (rectangle_index_bounds)
    int flags;     // bit 0: y part of getSubmap's success; bit 1: |y| usable (centre_usable); bit 2 (3x3-only kernels): jc == j0d + 1
    double ny;
    double sbaseY;   // submap position.y + (0.5 * sublength.y - 0.5 * res)
    double yA, yB;   // cell_pos(sbaseY, res, (rightCol + 1) >> 1), cell_pos(sbaseY, res, rightCol >> 1)  (cpp:1816)
    double dy2[3];   // (cell_pos(baseY, res, j0d + k) - ny)^2, k = 0..2 (3x3 disc form)
    // window columns (window origin jc - winH, one word) of the centroid rectangle [j0r, j0r + njr) and of the
    // reference rectangle polygon [jA, jB]
    uint32_t rmask, pmask;
};
static_assert(sizeof(YEntry) == 96, "YEntry layout");

// ds_swizzle of a double (bit mode), two dwords
template <int kPattern>
__device__ __forceinline__ double swizzle_f64(double v) {
    const long long bits = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_ds_swizzle(static_cast<int>(bits), kPattern);
    const int hi = __builtin_amdgcn_ds_swizzle(static_cast<int>(bits >> 32), kPattern);
    return __builtin_bit_cast(double, (static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

// Value of lane L (compile-time) of every 8-lane group: a ds_swizzle in bit mode.  (Two DPP moves instead — a quad broadcast,
// then the half-row mirror — were measured on the headline, round 4: 27.5 us either way; the exchange is not on the critical path.)
template <int L>
__device__ __forceinline__ int bcast8_dpp(int x) {
    return __builtin_amdgcn_ds_swizzle(x, 0x18 | (L << 5));
}
template <int L>
__device__ __forceinline__ double bcast8_dpp_f64(double v) {
    const long long bits = __builtin_bit_cast(long long, v);
    const int lo = bcast8_dpp<L>(static_cast<int>(bits)), hi = bcast8_dpp<L>(static_cast<int>(bits >> 32));
    return __builtin_bit_cast(double, (static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

// Multi-word row shifts by 0 <= s < 32 columns: shr: bit j of the result = bit j + s of the row; shl: bit j - s.
template <int KW>
__device__ __forceinline__ void row_shr(const unsigned (&x)[KW], unsigned s, unsigned (&o)[KW]) {
#pragma unroll
    for (int q = 0; q < KW; ++q) o[q] = __builtin_amdgcn_alignbit(q + 1 < KW ? x[q + 1] : 0u, x[q], s);
}
template <int KW>
__device__ __forceinline__ void row_shl(const unsigned (&x)[KW], unsigned s, unsigned (&o)[KW]) {
#pragma unroll
    for (int q = 0; q < KW; ++q) o[q] = s ? __builtin_amdgcn_alignbit(x[q], q > 0 ? x[q - 1] : 0u, 32u - s) : x[q];
}

__device__ __forceinline__ unsigned bits_from(int lo) { return lo >= 32 ? 0u : (lo <= 0 ? ~0u : (~0u << lo)); }
__device__ __forceinline__ unsigned bits_to(int hi) { return hi < 0 ? 0u : (hi >= 31 ? ~0u : ((2u << hi) - 1u)); }
// word `wi` of the mask with bits [lo, hi] set (bit positions over the whole multi-word row)
__device__ __forceinline__ unsigned range_word(int lo, int hi, int wi) { return bits_from(lo - 32 * wi) & bits_to(hi - 32 * wi); }

// Layer cell / plane word group at a 32-bit offset from the (uniform) base pointer: one 32-bit multiply-add instead
// of 64-bit address arithmetic per load.  bits_supported() bounds layers and planes below 2 GiB and 2^24 rows / columns.
__device__ __forceinline__ float load_cell(const float* base, unsigned cell) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + static_cast<size_t>(cell << 2));
}
__device__ __forceinline__ uint4 load_group(const uint4* base, unsigned group) {
    return *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(base) + static_cast<size_t>(group << 4));
}

// Window origin (iw0, jw0) = getIndex(centre) - winH.  Lane `sub` holds window rows sub + G * k.  Rows and word
// groups outside the map are clamped onto the zero padding of the planes.
template <int G, int NRL, int KW>
__device__ __forceinline__ void win_issue(const BitMap& bm, const MapGeom& mg, const Grp<G>& g, int iw0, int jw0,
                                          uint4 (&grp)[NRL][KW + 1]) {
    static_assert(KW + 1 <= kBitPadW, "the planes' zero padding must cover a whole window row");
    int w0 = jw0 >> 5;
    w0 = max(-kBitPadW, min(w0, bm.nw + kBitPadW - (KW + 1)));
#pragma unroll
    for (int k = 0; k < NRL; ++k) {
        int i = iw0 + g.sub + G * k;
        i = max(-1, min(i, mg.rows));
        // tile (row group, word) = one 128-byte line holding 8 consecutive rows: the lanes that own rows of one row
        // group read different 16-byte pieces of the SAME line (8-lane kernels: one or two lines per load instruction
        // instead of eight; one-wavefront-per-pose kernels: eight or nine instead of 64)
        const unsigned r1 = static_cast<unsigned>(i + 1);
        const unsigned first = ((__umul24(r1 >> 3, static_cast<unsigned>(bm.strideW)) + static_cast<unsigned>(w0 + kBitPadW)) << 3) + (r1 & 7u);
#pragma unroll
        for (int q = 0; q <= KW; ++q) grp[k][q] = load_group(bm.words, first + 8u * static_cast<unsigned>(q));
    }
}
template <int NRL, int KW>
__device__ __forceinline__ void win_finish(int jw0, const uint4 (&grp)[NRL][KW + 1], WinRows<NRL, KW>& w) {
    const unsigned sh = static_cast<unsigned>(jw0) & 31u;
#pragma unroll
    for (int k = 0; k < NRL; ++k)
#pragma unroll
        for (int q = 0; q < KW; ++q) {
            w.D[k][q] = __builtin_amdgcn_alignbit(grp[k][q + 1].x, grp[k][q].x, sh);
            w.Df[k][q] = __builtin_amdgcn_alignbit(grp[k][q + 1].y, grp[k][q].y, sh);
            w.C[k][q] = __builtin_amdgcn_alignbit(grp[k][q + 1].z, grp[k][q].z, sh);
            w.F[k][q] = __builtin_amdgcn_alignbit(grp[k][q + 1].w, grp[k][q].w, sh);
        }
}
// Bit (window row ri, window column cj) of a row array in LDS; 0 outside the window.
template <int KW>
__device__ __forceinline__ unsigned win_bit(const uint32_t* rows, int nRows, int ri, int cj) {
    const bool in = static_cast<unsigned>(ri) < static_cast<unsigned>(nRows) && static_cast<unsigned>(cj) < 32u * KW;
    const int r = min(max(ri, 0), nRows - 1), c = min(max(cj, 0), 32 * KW - 1);
    const uint32_t wd = rows[r * KW + (c >> 5)];
    return in ? (wd >> (c & 31)) & 1u : 0u;
}

// checkFootholdUseCentroidMethod's row scan (cpp:1649-1658 whole-region test, cpp:1717-1750 blocked rows) from the
// D rows: lane = window row.  `cnt > (rightCol + 1) * 0.5` (cpp:1743) is 2 * cnt > nj in integers.
template <int G, int NRL, int KW>
__device__ __forceinline__ CentroidScan rows_from_bits(const Submap& s, const WinRows<NRL, KW>& w, const Grp<G>& g, int iw0, int jw0,
                                                       const uint32_t* colMask = nullptr) {  // KW == 1: YEntry::rmask
    static_assert(G * NRL <= 128, "blocked-row masks are kept in two 64-bit words");
    CentroidScan r0;
    const int ni = s.ni, nj = s.nj;
    const int c0 = s.j0 - jw0, c1 = c0 + nj - 1;  // window columns of the rectangle
    unsigned long long blk[2] = {0ull, 0ull};      // bit = window row
    unsigned blk32 = 0u;                           // (windows of up to 32 rows: one 32-bit word)
    bool anyBelow = false;
#pragma unroll
    for (int k = 0; k < NRL; ++k) {
        const int ri = g.sub + G * k;
        const int r = iw0 + ri - s.i0;  // row of the rectangle held by this lane in slot k
        const bool liveRow = s.ok && r >= 0 && r < ni;
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < KW; ++q) cnt += __builtin_popcount(w.D[k][q] & (colMask ? *colMask : range_word(c0, c1, q)));
        anyBelow |= liveRow && cnt > 0;
        const bool blocked = liveRow && 2 * cnt > nj;
        const unsigned long long mk = g.ballot(blocked);
        if constexpr (G * NRL <= 32) {
            blk32 |= static_cast<unsigned>(mk) << (G * k);
        } else {
            static_assert(G == 64, "windows of more than 32 rows belong to the one-wavefront-per-pose kernels");
            blk[k & 1] |= mk;
        }
    }
    const int off = s.i0 - iw0;
    if constexpr (G * NRL <= 32) {  // the 8-lane shapes: 32-bit shifts and bit scans instead of 64-bit ones
        const unsigned rel = blk32 >> (off & 31);
        const unsigned relIn = (static_cast<unsigned>(off) < 32u) ? rel : 0u;
        r0.minRow = relIn ? __builtin_ctz(relIn) : 0;
        r0.maxRow = relIn ? 31 - __builtin_clz(relIn) : 0;
        r0.whole = s.ok && ni * nj > 0 && !g.any(anyBelow);
        return r0;
    }
    if constexpr (G * NRL <= 64) {  // the whole window in one word
        const unsigned long long rel = blk[0] >> (off & 63);
        const unsigned long long relIn = (static_cast<unsigned>(off) < 64u) ? rel : 0ull;
        r0.minRow = relIn ? __builtin_ctzll(relIn) : 0;
        r0.maxRow = relIn ? 63 - __builtin_clzll(relIn) : 0;
        r0.whole = s.ok && ni * nj > 0 && !g.any(anyBelow);
        return r0;
    }
    // rows relative to the rectangle's first row: a 128-bit shift (the rectangle lies inside the window, and a window
    // of more than 64 rows can hold a rectangle of more than 64)
    unsigned long long relLo = 0ull, relHi = 0ull;
    if (off >= 0 && off < 64) {
        relLo = (blk[0] >> off) | (off ? (blk[1] << (64 - off)) : 0ull);
        relHi = blk[1] >> off;
    } else if (off >= 64 && off < 128) {
        relLo = blk[1] >> (off - 64);
    }
    r0.minRow = relLo ? __builtin_ctzll(relLo) : (relHi ? 64 + __builtin_ctzll(relHi) : 0);
    r0.maxRow = relHi ? 127 - __builtin_clzll(relHi) : (relLo ? 63 - __builtin_clzll(relLo) : 0);
    r0.whole = s.ok && ni * nj > 0 && !g.any(anyBelow);
    return r0;
}

// checkDefaultFoothold (cpp:2039-2082) from the Df rows: valid iff >= 1 cell visited and no visited cell has its Df
// bit set.  The visited cells are the ones disc_issue() enumerated (d.vis / the 3x3 form); boxes it did not
// pipeline (clamped at the map border, or larger than the pipeline) are walked here, membership test included.
template <int G, int KW, bool kMid>
__device__ __forceinline__ bool default_ok_bits(const DevMap& m, const PlanConsts& pc, double cx, double cy, const BBox& bb,
                                                const DiscLoads& d, const uint32_t* rowsDf, int nRows, int iw0, int jw0, const Grp<G>& g) {
    bool any = false, fail = false;
    if (d.pipelined) {
        if (G == 8 && d.mid) {  // wave-uniform: cells 0-3 and 5-8 on the lanes, the middle cell always visited
            const int t = g.sub + (g.sub >= 4 ? 1 : 0);
            const int a = t >= 6 ? 2 : (t >= 3 ? 1 : 0);
            const int ri = bb.i0 - iw0, cj = bb.j0 - jw0;
            fail = (d.vis[0] != 0 && win_bit<KW>(rowsDf, nRows, ri + a, cj + (t - 3 * a)) != 0u) ||
                   win_bit<KW>(rowsDf, nRows, ri + 1, cj + 1) != 0u;
            return !g.any(fail);
        }
        if constexpr (!kMid) {
            const float njInv = rcp_small(bb.nj);
#pragma unroll
            for (int r = 0; r < disc_rounds<G>(); ++r) {
                // wave-uniform: a round past every box of the wavefront (64-bit rows: boxes of <= 64 cells; not worth a test on the 96-bit ones)
                if (KW <= 2 && r > 0 && __ballot(d.vis[r] != 0) == 0ull) continue;
                int a, bq;
                divmod_small(min(r * G + g.sub, 4095), max(bb.nj, 1), njInv, a, bq);
                const bool v = d.vis[r] != 0;
                any |= v;
                fail |= v && win_bit<KW>(rowsDf, nRows, bb.i0 + a - iw0, bb.j0 + bq - jw0) != 0u;
            }
            return g.any(any) && !g.any(fail);
        }
    }
    const int nb = bb.ni * bb.nj;
    const float njInv = rcp_small(bb.nj);
    for (int base = 0; base < nb; base += G) {
        const int t = base + g.sub;
        if (t < nb) {
            int a, bq;
            divmod_small(t, bb.nj, njInv, a, bq);
            const int i = bb.i0 + a, j = bb.j0 + bq;
            if (in_range(i, j, m.g.rows, m.g.cols) && cell_in_disc(m.g, i, j, cx, cy, pc.rf2)) {
                any = true;
                fail |= win_bit<KW>(rowsDf, nRows, i - iw0, j - jw0) != 0u;
            }
        }
    }
    return g.any(any) && !g.any(fail);
}

// Centroid case logic (cpp:1684-1952) given the row scan; the result's foot disc is cell-centred, i.e. the
// host-proved offset table in CircleIterator order, and getIndex(result) is top-left + (newRow, newCol).
// kOneCell: the 3x3-only variants run with a one-cell foot disc (rf < res): the result's height is that cell's, loaded
// here.  Otherwise the caller defers the result's height: flush_seqrec2 / flush_unit_g walk the offset table themselves.
struct CentroidPendingBits {
    CentroidOut o;
    int needDisc;  // 0/1
    float e0;      // kOneCell: elevation of the result's own cell
    // (e / vis: zero-filled below and read by nobody since the in-chain table walk went.  Without them the nine 3x3-only
    // kernels come out with two VGPR numbers exchanged — not an instruction more or fewer — and this code was cut down under
    // the condition that no kernel's instructions change: they go with the next change to those kernels.)
    float e[kDiscRounds];
    int vis[kDiscRounds];
};
// yA / yB (optional): the two possible result ordinates cell_pos(s.baseY, res, (rightCol + 1) >> 1) and
// cell_pos(s.baseY, res, rightCol >> 1), precomputed with the y side of the leg's geometry (YEntry).
template <bool kOneCell, bool kHaveY>
__device__ __forceinline__ void centroid_begin_bits_impl(const DevMap& m, const LegCtx& c, const Submap& s, const CentroidScan& sc,
                                                         float zCentre, CentroidPendingBits& cp, double yA, double yB) {
    CentroidOut& o = cp.o;
    cp.needDisc = 0;
    cp.e0 = 0.0f;
    o.x = 0.0;
    o.y = 0.0;
    o.z = 0.0f;
    o.row = -1;
    o.col = -1;
    o.code = 5;
#pragma unroll
    for (int r = 0; r < kDiscRounds; ++r) {
        cp.vis[r] = 0;
        cp.e[r] = 0.0f;
    }
    if (!s.ok) {  // cpp:1628-1631
        o.code = 6;
        return;
    }
    const int bottomRow = s.ni - 1, rightCol = s.nj - 1;
    const int minRow = sc.minRow, maxRow = sc.maxRow;
    if (sc.whole) {  // cpp:1684-1689
        o.x = c.cx;
        o.y = c.cy;
        o.z = zCentre;
        o.row = c.ici;
        o.col = c.icj;
        o.code = 0;
        return;
    }
    // floor((a) * 0.5) / ceil((a) * 0.5) of small non-negative integers, as integer arithmetic (exact)
    int newRow, newCol;
    if (minRow == 0 && maxRow != bottomRow) {  // case 1, cpp:1777-1786
        newRow = (maxRow + bottomRow + 1) >> 1;
        newCol = (rightCol + 1) >> 1;
        o.code = 1;
    } else if (minRow != 0 && maxRow != bottomRow) {  // case 2, cpp:1843-1886
        if ((minRow - 0) >= (bottomRow - maxRow)) {
            newRow = (minRow + 1) >> 1;
            o.code = 2;
        } else {
            newRow = (maxRow + bottomRow) >> 1;
            o.code = 3;
        }
        newCol = rightCol >> 1;
    } else if (minRow != 0 && maxRow == bottomRow) {  // case 3, cpp:1944-1952
        newRow = (minRow + 1) >> 1;
        newCol = rightCol >> 1;
        o.code = 4;
    } else {
        return;  // first and last row blocked: no branch taken, result stays (0,0,0)
    }
    o.x = cell_pos(s.baseX, m.g.res, newRow);  // map.getPosition(newIndex) on the SUBMAP (cpp:1816)
    if constexpr (kHaveY) o.y = (o.code == 1) ? yA : yB;
    else o.y = cell_pos(s.baseY, m.g.res, newCol);
    o.row = s.i0 + newRow;
    o.col = s.j0 + newCol;
    if constexpr (kOneCell) cp.e0 = m.elev[static_cast<size_t>(o.row) * m.g.cols + o.col];  // a cell of the submap: inside the map
    cp.needDisc = 1;
}
template <bool kOneCell>
__device__ __forceinline__ void centroid_begin_bits(const DevMap& m, const LegCtx& c, const Submap& s, const CentroidScan& sc, float zCentre,
                                                    CentroidPendingBits& cp) {
    centroid_begin_bits_impl<kOneCell, false>(m, c, s, sc, zCentre, cp, 0.0, 0.0);
}
template <bool kOneCell>
__device__ __forceinline__ void centroid_begin_bits(const DevMap& m, const LegCtx& c, const Submap& s, const CentroidScan& sc, float zCentre,
                                                    CentroidPendingBits& cp, double yA, double yB) {
    centroid_begin_bits_impl<kOneCell, true>(m, c, s, sc, zCentre, cp, yA, yB);
}

// The reference rectangle in index space.  Cell centres x_i = base + res * (-i) are non-increasing in i, so
// {i : lo <= x_i < hi} = [iA, iB] with iA = min{i : x_i < hi}, iB = max{i : x_i >= lo}; each end is found by evaluating
// the reference's own comparison at the two indices next to the boundary predicted by (base - limit) * (1/res).
// Lane q of the group evaluates one predicate (q & 4: y axis, q & 2: lower limit, q & 1: second index); the
// prediction e is read back from the even lanes.
struct IndexRect {
    int iA, iB, jA, jB;
};
template <int G>
__device__ __forceinline__ IndexRect rectangle_index_bounds(const MapGeom& mg, double xlo, double xhi, double ylo, double yhi,
                                                            const Grp<G>& g) {
    // (the limits arrive by value: a select between FIELDS of the leg context would keep the whole struct in scratch)
    const int q = g.sub & 7;
    const bool isY = (q & 4) != 0, isLo = (q & 2) != 0;
    const double base = isY ? mg.baseY : mg.baseX;
    const double lim = isY ? (isLo ? ylo : yhi) : (isLo ? xlo : xhi);
    double qf = floor((base - lim) * mg.rinv);
    qf = fmin(fmax(qf, -1.0e9), 1.0e9);
    const int e = static_cast<int>(qf);
    // upper limit: P(e), P(e + 1) with P(i) = x_i < hi;  lower limit: Q(e + 1), Q(e) with Q(i) = x_i >= lo
    const int t = isLo ? e + 1 - (q & 1) : e + (q & 1);
    const double x = cell_pos(base, mg.res, t);
    const bool pred = isLo ? (x >= lim) : (x < lim);
    const unsigned b = static_cast<unsigned>(g.ballot(pred && g.sub < 8));
    const int eXhi = g.template bcast_c<0>(e), eXlo = g.template bcast_c<2>(e), eYhi = g.template bcast_c<4>(e), eYlo = g.template bcast_c<6>(e);
    IndexRect r;
    r.iA = (b & 1u) ? eXhi : ((b & 2u) ? eXhi + 1 : eXhi + 2);
    r.iB = (b & 4u) ? eXlo + 1 : ((b & 8u) ? eXlo : eXlo - 1);
    r.jA = (b & 16u) ? eYhi : ((b & 32u) ? eYhi + 1 : eYhi + 2);
    r.jB = (b & 64u) ? eYlo + 1 : ((b & 128u) ? eYlo : eYlo - 1);
    return r;
}

// Arbitrary polygons on the multi-word windows.  PNPOLY (Polygon::isInside, cpp:2138) counts, for a cell centre
// (px, py), the edges straddling py whose intersection abscissa lies beyond px; py and therefore the abscissae depend
// on the window COLUMN only (see column_crossings above).  With at most two crossings X0, X1 per column a cell is
// inside iff (px < X0) != (px < X1), and since cell centres px_i are non-increasing in the row index i each
// comparison is a row threshold t(X) = min{i : px_i < X} (found exactly, as in rectangle_index_bounds): column c is
// inside for the rows [min(t0, t1), max(t0, t1)).  Lane = column; writes (lo, hi) per column.  Returns false when
// some column has more than two crossings (non-convex polygon): the per-cell PNPOLY loop is then used.
// The columns [colLo, colHi] only (those a candidate's foot disc can touch), and each column sets its bits in the
// "enters" / "leaves" row arrays itself (see the caller): the interval stays in the lane's registers.
template <int G, int KW>
__device__ __forceinline__ bool window_column_rows(const MapGeom& mg, const LegCtx& c, const Grp<G>& g, int iw0, int jw0, int colLo, int colHi,
                                                   int NR, uint32_t* entersAt, uint32_t* leavesAt) {
    const double ninf = -__builtin_huge_val();
    bool over = false;
    for (int b = colLo + g.sub; b <= colHi; b += G) {
        const double py = cell_pos(mg.baseY, mg.res, jw0 + b);
        double X[2] = {ninf, ninf};
        // the (at most two) edges that straddle py, found with comparisons only; their abscissae afterwards — two division
        // sequences per column pass instead of one per polygon edge (the lanes' columns straddle different edges)
        int n = 0, e0 = 0, e1 = 0;
        for (int i = 0, j = c.nv - 1; i < c.nv; j = i++) {
            const bool cross = (c.vy[i] > py) != (c.vy[j] > py);
            e1 = (cross && n == 1) ? i : e1;
            e0 = (cross && n == 0) ? i : e0;
            n += cross ? 1 : 0;
        }
        over |= n > 2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (n > u) {
                const int i = u == 0 ? e0 : e1;
                const int j = i == 0 ? c.nv - 1 : i - 1;
                const double vxi = c.vx[i], vyi = c.vy[i], vxj = c.vx[j], vyj = c.vy[j];
                const double ex = vxj - vxi;
                const double t = py - vyi;
                double xi = vxi;
                if (!(ex == 0.0 && fabs(t) <= DBL_MAX)) xi = ex * t / (vyj - vyi) + vxi;  // polygon_inside_fast
                X[u] = xi;
            }
        }
        int t[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            double qf = floor((mg.baseX - X[u]) * mg.rinv);
            qf = fmin(fmax(qf, -1.0e9), 1.0e9);
            const int e = static_cast<int>(qf);
            const bool p0 = cell_pos(mg.baseX, mg.res, e) < X[u], p1 = cell_pos(mg.baseX, mg.res, e + 1) < X[u];
            t[u] = p0 ? e : (p1 ? e + 1 : e + 2);
        }
        const int rl = min(t[0], t[1]) - iw0, rh = max(t[0], t[1]) - iw0;  // window rows [rl, rh)
        const uint32_t bit = 1u << (b & 31);
        const int wq = b >> 5;
        if (rl < rh && rh > 0 && rl < NR) {
            atomicOr(&entersAt[max(rl, 0) * KW + wq], bit);
            if (rh < NR) atomicOr(&leavesAt[rh * KW + wq], bit);
        }
    }
    return !g.any(over);
}

// Inclusive OR-scan over the 64 lanes of a wavefront (lane l gets the OR of lanes 0..l): four shifts inside the 16-lane
// DPP rows, then the last lane of a row into the next row, then lane 31 into the upper half.
__device__ __forceinline__ unsigned wave_or_scan(unsigned v) {
    int x = static_cast<int>(v);
    x |= __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);   // row_shr:1
    x |= __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);   // row_shr:2
    x |= __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);   // row_shr:4
    x |= __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);   // row_shr:8
    x |= __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1 and 3
    x |= __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2 and 3
    return static_cast<unsigned>(x);
}

// Distance (columns) from window column cj to the nearest set bit of a row of KW words; >= 1 << 20 when the row is empty.
template <int KW>
__device__ __forceinline__ int nearest_set_bit_distance(const uint32_t* row, int cj) {
    int best = 1 << 20;
#pragma unroll
    for (int q = 0; q < KW; ++q) {
        const int rel = cj - 32 * q;  // the centre column relative to this word
        const unsigned left = row[q] & bits_to(rel), right = row[q] & bits_from(rel);
        const int dl = left ? rel - (31 - __builtin_clz(left)) : (1 << 20);
        const int dr = right ? __builtin_ctz(right) - rel : (1 << 20);
        best = min(best, min(dl, dr));
    }
    return best;
}
// Minimum of a small non-negative value (< 128; larger values count as 127) over the lanes of a group, by ballots.
template <int G>
__device__ __forceinline__ int group_min7(const Grp<G>& g, int v) {
    v = min(v, 127);
    unsigned long long cand = g.ballot(true);
    int r = 0;
#pragma unroll
    for (int b = 6; b >= 0; --b) {
        const unsigned long long zero = g.ballot(((v >> b) & 1) == 0) & cand;
        if (zero) cand = zero;
        else r |= 1 << b;
    }
    return r;
}

// H_d(x): bit j = AND_{|t| <= d} x bit j + t (zeros beyond the row's words), by doubling: x & x>>1, & >>2, ... then centred
template <int KW>
__device__ __forceinline__ void erode_h(unsigned (&A)[KW], int d) {
    if (d <= 0) return;
    const int L = 2 * d + 1;
    unsigned T[KW];
    int span = 1;
    while (2 * span <= L) {  // A covers columns [j, j + span)
        row_shr<KW>(A, static_cast<unsigned>(span), T);
#pragma unroll
        for (int q = 0; q < KW; ++q) A[q] &= T[q];
        span *= 2;
    }
    if (span < L) {
        row_shr<KW>(A, static_cast<unsigned>(L - span), T);
#pragma unroll
        for (int q = 0; q < KW; ++q) A[q] &= T[q];
    }
    row_shl<KW>(A, static_cast<unsigned>(d), T);  // centre the interval: [j - d, j + d]
#pragma unroll
    for (int q = 0; q < KW; ++q) A[q] = T[q];
}

// checkCandidateFoothold (cpp:2085-2114) on the window's bit rows: first valid cell in SpiralIterator order.
// kOneCellFoot: the caller is a 3x3-only kernel, launched for one-cell foot discs only (select_plan_kernel): the erosion
// is compiled out (its code and live scalars cost the chain of those kernels 1 us of register allocation otherwise).
template <int G, int NRL, int KW, bool kOneCellFoot = false>
__device__ bool spiral_bits(const DevMap& m, const PlanConsts& pc, const SpiralLut& lut, const LutHead& head, const LegCtx& c,
                            const WinRows<NRL, KW>& w, const LegBits& lb, const Grp<G>& g, int iw0, int jw0, int& wi, int& wj,
                            const YEntry* ye = nullptr) {
    const int NR = lb.rows;  // allocated window rows (lanes beyond them hold nothing a search can touch)
    // Every candidate has |di|, |dj| <= nRings.  A centre so far off the map that none of them is inside it — poses that
    // walked off the map, or a feet polygon degenerated by the centroid track's "no case" (0,0,0) results — has no valid
    // candidate; without this test such a leg scans every round with in_range false, in every phase of every remaining
    // cycle (cfg-3: 122 of a pose's 128 searches, 1.3 of its 2.5 M clocks, and the kernel waits for its slowest pose).
    if (c.ici + c.nRings < 0 || c.ici - c.nRings >= m.g.rows || c.icj + c.nRings < 0 || c.icj - c.nRings >= m.g.cols) return false;
    // generic 8-lane kernels: the first round's table entries are requested here, ahead of the P rows and the erosion
    uint4 tabFirst = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (G == 8 && KW == 1 && !kOneCellFoot) tabFirst = reinterpret_cast<const uint4*>(lut.packed)[g.sub];
    // Window rows sized for the largest search radius a pose may ask for (fpe_set_max_leg_search_radius) are beyond the reach
    // of a leg with the usual radius: when every row such a leg's candidates and their foot discs can touch is held in the
    // lanes' FIRST row (one-wavefront-per-pose kernels with two rows per lane), the second row's share of the P rows, the
    // erosion and the ring skip is not computed at all (cfg-5: half of those stages)
    const int kLim = (G == 64 && NRL > 1 && pc.winH + c.nRings + pc.footReach < G) ? 1 : NRL;
    bool polyFolded = true;  // the polygon test is part of P (rectangle: always; other polygons: see below)
    unsigned Preg[NRL];      // single-word rows: this lane's P rows stay in registers for the erosion
#pragma unroll
    for (int k = 0; k < NRL; ++k) Preg[k] = 0u;
    // (1) per row: P = cells that do NOT fail checkCirclePolygonFoothold's per-cell test (cpp:2132-2138)
    if (c.rect) {
        IndexRect ir = rectangle_index_bounds(m.g, c.xlo, c.xhi, c.ylo, c.yhi, g);
        if (ye) {  // the column interval is chain-independent: taken from the hoisted y side (same evaluation)
            ir.jA = ye->jA;
            ir.jB = ye->jB;
        }
#pragma unroll
        for (int k = 0; k < NRL; ++k) {
            if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
            const int ri = g.sub + G * k;
            const int i = iw0 + ri;
            const bool rowIn = i >= ir.iA && i <= ir.iB;
#pragma unroll
            for (int q = 0; q < KW; ++q) {
                const unsigned inside = rowIn ? ((ye && KW == 1) ? ye->pmask : range_word(ir.jA - jw0, ir.jB - jw0, q)) : 0u;
                if (ri < NR) lb.a[ri * KW + q] = ~w.F[k][q] | (~w.C[k][q] & inside);
                if constexpr (KW == 1) Preg[k] = ~w.F[k][0] | (~w.C[k][0] & inside);
            }
        }
    } else {
        bool folded = false;
        if constexpr (KW > 1) {
            static_assert(G == 64, "the column -> row transposition runs on whole wavefronts");
            // the polygon's row interval per window column (lane = column), then transposed into per-row column
            // masks by ballots over the columns, one window row at a time
            uint32_t* entersAt = lb.f;
            uint32_t* leavesAt = lb.h0;
            for (int idx = g.sub; idx < NR * KW; idx += G) {
                entersAt[idx] = 0u;
                leavesAt[idx] = 0u;
            }
            bits_sync<G>();
            // columns a candidate's foot disc can touch: within nRings + footReach of the centre column (winH) — one pass of
            // the wavefront instead of two for the usual radius on a 96-bit window
            const int reachCols = min(c.nRings + pc.footReach, pc.winH);
            folded = window_column_rows<G, KW>(m.g, c, g, iw0, jw0, max(pc.winH - reachCols, 0), min(pc.winH + reachCols, 32 * KW - 1), NR,
                                               entersAt, leavesAt);
            if (folded) {
                // Column intervals -> row masks without a ballot per row.  Column c is inside for the rows [lo_c, hi_c): it
                // ENTERS at row lo_c and LEAVES at row hi_c.  Each column sets its bit in the "enters" word of its first
                // row and in the "leaves" word of its end row (LDS atomic OR; two scratch row arrays that are free here);
                // an inclusive OR-scan over the rows (lane = row: four row shifts and two row broadcasts per word) then
                // gives, for every row, the columns that have entered and the columns that have left:
                //     inside(row) = entered(row) & ~left(row)
                // — the same set as the per-row comparison i >= lo_c && i < hi_c, by construction.
                bits_sync<G>();
                unsigned inside[NRL][KW];
                // rows a candidate's foot disc can touch: within nRings + footReach rows of the centre row (winH)
                const int reachRows = min(c.nRings + pc.footReach, pc.winH);
                const int rowLo = pc.winH - reachRows, rowHi = min(pc.winH + reachRows + 1, NR);  // NR: allocated rows
                unsigned carryIn[KW], carryOut[KW];
#pragma unroll
                for (int q = 0; q < KW; ++q) carryIn[q] = carryOut[q] = 0u;
#pragma unroll
                for (int k = 0; k < NRL; ++k) {
                    if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
                    const int ri = g.sub + G * k;
#pragma unroll
                    for (int q = 0; q < KW; ++q) {
                        unsigned en = ri < NR ? entersAt[ri * KW + q] : 0u, lv = ri < NR ? leavesAt[ri * KW + q] : 0u;
                        en = wave_or_scan(en) | carryIn[q];
                        lv = wave_or_scan(lv) | carryOut[q];
                        carryIn[q] = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(en), 63));
                        carryOut[q] = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(lv), 63));
                        inside[k][q] = (ri >= rowLo && ri < rowHi) ? (en & ~lv) : 0u;
                    }
                }
#pragma unroll
                for (int k = 0; k < NRL; ++k) {
                    if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
                    const int ri = g.sub + G * k;
#pragma unroll
                    for (int q = 0; q < KW; ++q)
                        if (ri < NR) lb.a[ri * KW + q] = ~w.F[k][q] | (~w.C[k][q] & inside[k][q]);
                }
            }
        }
        polyFolded = folded;
        if (!folded) {
#pragma unroll
            for (int k = 0; k < NRL; ++k) {
                if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
                const int ri = g.sub + G * k;
#pragma unroll
                for (int q = 0; q < KW; ++q) {
                    if (ri >= NR) continue;
                    lb.a[ri * KW + q] = ~w.C[k][q];  // threshold only (C implies F); the polygon is tested per candidate below
                    lb.f[ri * KW + q] = w.F[k][q];
                    if constexpr (KW == 1) Preg[k] = ~w.C[k][0];
                }
            }
        }
    }
    bits_sync<G>();
    // (2) erosion with the foot-disc offset table: E bit (row, col) = AND_k P(row + da_k, col + db_k)
    const uint32_t* E = lb.a;
    if (!kOneCellFoot && pc.nFoot > 1 && pc.nHW > 0) {
        // the two small tables in registers, fetched once (indexed inside the loops below they are a scalar load and a
        // wait per iteration): hwList[4] as one word, hwIdx[16] as two
        uint32_t hwListW;
        unsigned long long hwIdxLo, hwIdxHi;
        __builtin_memcpy(&hwListW, pc.hwList, 4);
        __builtin_memcpy(&hwIdxLo, pc.hwIdx, 8);
        __builtin_memcpy(&hwIdxHi, pc.hwIdx + 8, 8);
        // row-interval form: the disc's row +-a holds the columns [-w(a), w(a)], so
        //   E(row) = AND_a H_w(a)(P(row + a)) & H_w(a)(P(row - a)),   H_w(x) bit j = AND_{|t| <= w} x bit j + t
        // — a handful of shifts per distinct width instead of one shift per offset (45 offsets on a 0.5 cm map)
        if constexpr (KW == 1) {
            // single-word rows (8-lane kernels; measured against the nested form below: cfg-4 -2.5 %): H_w of this lane's
            // rows straight from the registers, H_w(x) = AND_{|t| <= w} x shifted by t, one array per distinct width ...
            for (int hw = 0; hw < pc.nHW; ++hw) {
                const int wdt = static_cast<int>((hwListW >> (8 * hw)) & 0xFFu);
                unsigned acc[NRL];
#pragma unroll
                for (int k = 0; k < NRL; ++k) acc[k] = Preg[k];
                for (int t = 1; t <= wdt; ++t) {
#pragma unroll
                    for (int k = 0; k < NRL; ++k) acc[k] &= (Preg[k] >> t) & (Preg[k] << t);
                }
#pragma unroll
                for (int k = 0; k < NRL; ++k)
                    if (g.sub + G * k < NR) lb.h0[hw * lb.hStride + g.sub + G * k] = acc[k];
            }
            bits_sync<G>();
            // ... then the rows +-a of the array of w(a) (a outermost: the reads of all of this lane's rows are in flight together)
            unsigned e[NRL];
#pragma unroll
            for (int k = 0; k < NRL; ++k) e[k] = ~0u;
            for (int a = 0; a <= pc.footReach; ++a) {
                const int hwOfRow = static_cast<int>(((a < 8 ? hwIdxLo : hwIdxHi) >> (8 * (a & 7))) & 0xFFu);
                const uint32_t* hrow = lb.h0 + hwOfRow * lb.hStride;
#pragma unroll
                for (int k = 0; k < NRL; ++k) {
                    const int ri = g.sub + G * k;
                    e[k] &= hrow[min(max(ri - a, 0), NR - 1)] & hrow[min(max(ri + a, 0), NR - 1)];
                }
            }
#pragma unroll
            for (int k = 0; k < NRL; ++k)
                if (g.sub + G * k < NR) lb.a[g.sub + G * k] = e[k];  // the P rows are dead: E takes their place
        } else {
            // Multi-word rows, vertical first: H_w distributes over AND and H_a(H_b(x)) = H_(a + b)(x) (zero fill included),
            // and a disc's widths do not grow with |a| (derive_foot_offsets checks it), so with V_q = AND of the rows
            // P(row +- a) whose width is the q-th distinct one, w_0 > w_1 > ...:
            //   E = H_w0(V_0) & H_w1(V_1) & ... = H_w(n-1)( ... H_(w1 - w2)( H_(w0 - w1)(V_0) & V_1 ) & V_2 ... )
            // — the rows are ANDed as they are read (no intermediate arrays, no second pass), and the horizontal work is
            // w_0 single steps per row in total instead of one full H_w per distinct width (cfg-5: -5 %).
            unsigned acc[NRL][KW];
#pragma unroll
            for (int k = 0; k < NRL; ++k)
#pragma unroll
                for (int q = 0; q < KW; ++q) acc[k][q] = ~0u;
            int curW = static_cast<int>(hwListW & 0xFFu);  // w(0): hwIdx[0] == 0 by construction
            for (int a = 0; a <= pc.footReach; ++a) {
                const int hwOfRow = static_cast<int>(((a < 8 ? hwIdxLo : hwIdxHi) >> (8 * (a & 7))) & 0xFFu);
                const int wa = static_cast<int>((hwListW >> (8 * hwOfRow)) & 0xFFu);
                if (wa != curW) {  // uniform: the next (narrower) group of rows
#pragma unroll
                    for (int k = 0; k < NRL; ++k) {
                        if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
                        erode_h<KW>(acc[k], curW - wa);
                    }
                    curW = wa;
                }
#pragma unroll
                for (int k = 0; k < NRL; ++k) {
                    if (k >= kLim) continue;
                    const int ri = g.sub + G * k;
                    const uint32_t* up = lb.a + min(max(ri - a, 0), NR - 1) * KW;
                    const uint32_t* dn = lb.a + min(max(ri + a, 0), NR - 1) * KW;
#pragma unroll
                    for (int q = 0; q < KW; ++q) acc[k][q] &= up[q] & dn[q];
                }
            }
#pragma unroll
            for (int k = 0; k < NRL; ++k) {
                if (k >= kLim) continue;
                const int ri = g.sub + G * k;
                erode_h<KW>(acc[k], curW);
#pragma unroll
                for (int q = 0; q < KW; ++q)
                    if (ri < NR) lb.h0[ri * KW + q] = acc[k][q];
            }
            E = lb.h0;
        }
        bits_sync<G>();
    } else if (!kOneCellFoot && pc.nFoot > 1) {
#pragma unroll
        for (int k = 0; k < NRL; ++k) {
            if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
            const int ri = g.sub + G * k;
            unsigned e[KW];
#pragma unroll
            for (int q = 0; q < KW; ++q) e[q] = ~0u;
            for (int f = 0; f < pc.nFoot; ++f) {
                const int da = c.footDa[f], db = c.footDb[f];
                const uint32_t* p = lb.a + min(max(ri + da, 0), NR - 1) * KW;
                // shift the row by db columns (|db| <= footReach < 32): bit j of the result = bit j + db of the row
#pragma unroll
                for (int q = 0; q < KW; ++q) {
                    const unsigned cur = p[q];
                    const unsigned up = q + 1 < KW ? p[q + 1] : 0u, dn = q > 0 ? p[q - 1] : 0u;
                    const unsigned sh = db >= 0 ? __builtin_amdgcn_alignbit(up, cur, static_cast<unsigned>(db))
                                                : __builtin_amdgcn_alignbit(cur, dn, static_cast<unsigned>(32 + db));
                    e[q] &= sh;
                }
            }
#pragma unroll
            for (int q = 0; q < KW; ++q)
                if (ri < NR) lb.h0[ri * KW + q] = e[q];
        }
        bits_sync<G>();
        E = lb.h0;
    }
    // Forms of the candidate scan, chosen per kernel shape by measurement (A/B on the BASELINE configurations): the
    // one-wavefront-per-pose kernels (64- and 96-bit rows) take straight-line rounds of 64 candidates with the ring skip
    // (cfg-5: 0.98 -> 0.76 ms in round 2); the generic 8-lane kernels four packed table entries per lane and round (below); the
    // 3x3-only 8-lane kernels, which come here only for ranks beyond their own first sixteen, the straight-line rounds
    // without the skip.
    constexpr bool kRingSkip = KW >= 2;
    if constexpr (G == 8 && KW == 1 && !kOneCellFoot) {
        // (3) generic 8-lane kernels (the 3x3-only ones evaluate ranks 0-15 in leg_fast8m and come here for the rest; the
        // scan below cost them registers: measured +3 % on the headline): FOUR candidates per lane and round (rank k = 32 * round + 4 * lane + u, one uint4 of packed
        // table entries per lane), so the first valid cell in spiral order is the lowest (lane, u) with a pass bit.  A
        // candidate lies within nRings <= winH rows and columns of the window's centre: its E bit is read without range
        // tests; cells outside the map are cleared from E first (wave-uniform, windows at the map's border only).
        const int M = c.nCand;
        const int rowW = c.ici - iw0, colW = c.icj - jw0;  // the centre inside the window: (winH, winH)
        uint32_t* Ew = const_cast<uint32_t*>(E);
        const bool border = iw0 < 0 || jw0 < 0 || iw0 + NR > m.g.rows || jw0 + 32 > m.g.cols;
        if (__ballot(border) != 0ull) {
            const uint32_t colIn = range_word(-jw0, m.g.cols - 1 - jw0, 0);
#pragma unroll
            for (int k = 0; k < NRL; ++k) {
                if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
                const int ri = g.sub + G * k;
                if (ri < NR) Ew[ri] = static_cast<unsigned>(iw0 + ri) < static_cast<unsigned>(m.g.rows) ? (Ew[ri] & colIn) : 0u;
            }
            bits_sync<G>();
        }
        const uint4* tab = reinterpret_cast<const uint4*>(lut.packed);
        const int nRounds = (M + 31) >> 5;
        uint4 nxt = tabFirst;
        for (int round = 0; round < nRounds; ++round) {
            const uint4 cur = nxt;
            nxt = tab[(round + 1) * G + g.sub];  // (the table is padded by one round)
            const uint32_t wds[4] = {cur.x, cur.y, cur.z, cur.w};
            const int k0 = round * 32 + 4 * g.sub;
            bool ok[4], outer[4];
            bool anyOuterOk = false;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool liveU = k0 + u < M;
                const int di = static_cast<int8_t>(wds[u] & 0xFFu), dj = static_cast<int8_t>((wds[u] >> 8) & 0xFFu);
                const int r = static_cast<int>((wds[u] >> 16) & 0xFFu);
                const uint32_t row = Ew[liveU ? rowW + di : 0];  // (entries beyond this leg's radius may point outside the window)
                ok[u] = liveU & (((row >> ((colW + dj) & 31)) & 1u) != 0u);
                // SpiralIterator::generateRing filters rings nRings-1 and nRings by isInside; the centre cell (ring 0) is
                // pushed unfiltered by the constructor
                outer[u] = (r >= 1) & (r + 1 >= c.nRings);
                anyOuterOk |= ok[u] & outer[u];
            }
            if (__ballot(anyOuterOk) != 0ull) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int di = static_cast<int8_t>(wds[u] & 0xFFu), dj = static_cast<int8_t>((wds[u] >> 8) & 0xFFu);
                    if (ok[u] & outer[u]) ok[u] = cell_in_disc(m.g, c.ici + di, c.icj + dj, c.cx, c.cy, c.R2);
                }
            }
            if (!polyFolded && __ballot(ok[0] | ok[1] | ok[2] | ok[3]) != 0ull) {
                // arbitrary polygon not folded into P: every FINITE cell of the foot disc must lie inside it (cpp:2138)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!ok[u]) continue;
                    const int i = c.ici + static_cast<int8_t>(wds[u] & 0xFFu), j = c.icj + static_cast<int8_t>((wds[u] >> 8) & 0xFFu);
                    for (int f = 0; f < pc.nFoot; ++f) {
                        const int qi = i + c.footDa[f], qj = j + c.footDb[f];
                        if (win_bit<KW>(lb.f, NR, qi - iw0, qj - jw0) == 0u) continue;
                        if (!polygon_inside_fast(c.vx, c.vy, c.nv, cell_pos(m.g.baseX, m.g.res, qi), cell_pos(m.g.baseY, m.g.res, qj))) {
                            ok[u] = false;
                            break;
                        }
                    }
                }
            }
            const unsigned mask = static_cast<unsigned>(g.ballot(ok[0] | ok[1] | ok[2] | ok[3]));
            if (mask) {
                const uint32_t mine = ok[0] ? wds[0] : (ok[1] ? wds[1] : (ok[2] ? wds[2] : wds[3]));
                const uint32_t win = g.bcast(mine, __builtin_ctz(mask));
                wi = c.ici + static_cast<int8_t>(win & 0xFFu);
                wj = c.icj + static_cast<int8_t>((win >> 8) & 0xFFu);
                return true;
            }
        }
    } else {
        // (3) candidates in rank order, lane = rank; lowest set ballot bit = argmin of rank.  Straight-line per round
        // (per-lane `if` chains are compiled into exec-mask branches): lanes beyond the table and cells outside the map carry
        // ok = false through unconditional, clamped evaluations; the disc filter of the outer rings and the per-candidate
        // polygon test of an unfolded polygon sit behind wave-uniform branches.
        const int M = c.nCand;
        // (2b) Where the scan can start.  A candidate needs its E bit, and the iterator's ring of a cell is
        // trunc(sqrt(di^2 + dj^2)) (fpe_host.cpp::build_spiral_table): the nearest E bit of every window row (lane = row)
        // gives the lowest ring rho that holds any E bit at all.  Ranks below ringStart[rho] cannot be valid: the scan
        // starts at the round containing ringStart[rho], and a window without an E bit inside the search radius has no
        // candidate — the searches that used to walk every round to the end (a pose stuck on bad terrain repeats them in
        // every remaining cycle; with one wavefront per pose such poses set the kernel's duration).
        int startBase = 0;
        bool nearHit = false;
        if constexpr (kRingSkip) {
            // the usual search has a pass bit within three rows and columns of the centre (ring <= 4: among the first 49
            // ranks, i.e. in the first round of 64): one ballot spares it the ring computation below
            bool near = false;
#pragma unroll
            for (int k = 0; k < NRL; ++k) {
                if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
                const int ri = g.sub + G * k;
                const int cj = c.icj - jw0;
                uint32_t bits = 0u;
#pragma unroll
                for (int q = 0; q < KW; ++q)
                    bits |= E[min(ri, NR - 1) * KW + q] & range_word(max(cj - 3, -jw0), min(cj + 3, m.g.cols - 1 - jw0), q);
                near |= ri < NR && abs(ri - (c.ici - iw0)) <= 3 && bits != 0u && static_cast<unsigned>(iw0 + ri) < static_cast<unsigned>(m.g.rows);
            }
            nearHit = g.any(near);
        }
        if (kRingSkip && !nearHit) {
            int ringRow = 1 << 20;
#pragma unroll
            for (int k = 0; k < NRL; ++k) {
                if (k >= kLim) continue;  // (rows no candidate of this leg can touch)
                const int ri = g.sub + G * k;
                const int a = abs(ri - (c.ici - iw0));
                uint32_t rowIn[KW];  // the row's E bits on columns inside the map (cells outside it pass every test but are no candidates)
#pragma unroll
                for (int q = 0; q < KW; ++q) rowIn[q] = E[min(ri, NR - 1) * KW + q] & range_word(-jw0, m.g.cols - 1 - jw0, q);
                const bool rowInMap = static_cast<unsigned>(iw0 + ri) < static_cast<unsigned>(m.g.rows);
                const int d = rowInMap ? nearest_set_bit_distance<KW>(rowIn, c.icj - jw0) : (1 << 20);
                const int n2 = a * a + d * d;  // <= 2 * 127^2 when in reach: exact in f32
                int rr = static_cast<int>(__builtin_sqrtf(static_cast<float>(min(n2, 1 << 16))));
                rr = (rr + 1) * (rr + 1) <= n2 ? rr + 1 : rr;  // v_sqrt_f32 is 1 ulp: settle floor(sqrt(n2)) exactly
                rr = rr * rr > n2 ? rr - 1 : rr;
                if (ri < NR && d < (1 << 20)) ringRow = min(ringRow, rr);
            }
            const int rho = group_min7<G>(g, ringRow);
            if (rho > c.nRings) return false;
            if (__ballot(rho >= 2) != 0ull) {  // uniform: the usual search (a pass bit in rings 0-1) needs no table lookup
                const int first = lut.ringStart[min(rho, lut.maxRing)];
                startBase = rho >= 2 ? (first / G) * G : 0;
            }
        }
        int round = startBase / G;
        int nDi = 0, nDj = 0, nR = c.nRings;
        if (__ballot(round >= kLutHeadRounds) != 0ull) {  // uniform: a late start reads its first round's entries here
            const int kn = min(startBase + g.sub, M - 1);
            nDi = lut.di[kn];
            nDj = lut.dj[kn];
            nR = lut.ring[kn];
        }
        for (int base = startBase; base < M; base += G, ++round) {
            const int k = base + g.sub;
            const bool live = k < M;
            int di, dj, r;
            if (round < kLutHeadRounds) {  // uniform
                const int e = round == 0 ? head.dij[0] : head.dij[1];
                di = static_cast<int16_t>(e & 0xFFFF);
                dj = e >> 16;
                r = round == 0 ? head.ring[0] : head.ring[1];
            } else {
                di = nDi;
                dj = nDj;
                r = nR;
            }
            if (round + 1 >= kLutHeadRounds) {
                // uniform: the next round's table entries, untouched until then (their latency is this round's work);
                // clamped index instead of a lane-dependent branch
                const int kn = min(k + G, M - 1);
                nDi = lut.di[kn];
                nDj = lut.dj[kn];
                nR = lut.ring[kn];
            }
            const int i = c.ici + di, j = c.icj + dj;
            bool ok = live & in_range(i, j, m.g.rows, m.g.cols);
            // SpiralIterator::generateRing filters rings nRings-1 and nRings by isInside; the centre cell (ring 0) is
            // pushed unfiltered by the constructor
            const bool outer = (r >= 1) & ((r == c.nRings) | (r + 1 == c.nRings));
            if (__ballot(ok & outer) != 0ull) {
                const bool inDisc = cell_in_disc(m.g, i, j, c.cx, c.cy, c.R2);
                ok = ok & (!outer | inDisc);
            }
            ok = ok & (win_bit<KW>(E, NR, i - iw0, j - jw0) != 0u);
            if (!polyFolded && __ballot(ok) != 0ull) {
                if (ok) {
                    // arbitrary polygon not folded into P: every FINITE cell of the foot disc must lie inside it (cpp:2138)
                    for (int f = 0; f < pc.nFoot; ++f) {
                        const int qi = i + c.footDa[f], qj = j + c.footDb[f];
                        if (win_bit<KW>(lb.f, NR, qi - iw0, qj - jw0) == 0u) continue;
                        if (!polygon_inside_fast(c.vx, c.vy, c.nv, cell_pos(m.g.baseX, m.g.res, qi), cell_pos(m.g.baseY, m.g.res, qj))) {
                            ok = false;
                            break;
                        }
                    }
                }
            }
            const unsigned long long mask = g.ballot(ok);
            if (mask) {
                const int l = __builtin_ctzll(mask);
                wi = g.bcast(i, l);
                wj = g.bcast(j, l);
                return true;
            }
        }
    }
    return false;
}

// Two mean heights side by side — a disc around a known centre (bounding box + membership mask) and, optionally, a
// cell-centred disc (offset table) — with the loads of both in ONE batch per eight cells.  Each sum is the ordered f32 sum
// of getFootholdMeanHeight (cpp:2520-2554): visited cells in CircleIterator (row-major) order, non-finite values count as 0,
// values >= 10 are skipped, finish_mean divides (or falls back on the last visited value).
struct MeanAcc {
    float sum, last;
    int cnt;
};
__device__ __forceinline__ void mean_acc(MeanAcc& a, bool vis, float e) {
    const float v = __builtin_isfinite(e) ? e : 0.0f;  // cpp:2532-2537
    const bool inc = vis && v < 10;                     // cpp:2539
    a.last = vis ? v : a.last;
    a.cnt += inc ? 1 : 0;
    a.sum = a.sum + (inc ? v : -0.0f);  // s + (-0.0f) == s for every s
}
// NA box cells and NC table entries per batch (one dependent round trip per batch)
template <int NA, int NC>
__device__ __forceinline__ void seq_mean2(const float* __restrict__ elev, int rows, int cols, int i0, int j0, int nj, unsigned long long v0,
                                          unsigned long long v1, bool wantC, int cRow, int cCol, const int8_t* da, const int8_t* db, int nFoot,
                                          double h, float& zBox, float& zC) {
    static_assert(NC == 8, "the offset table is read eight entries (two 64-bit LDS words) at a time");
    MeanAcc A{0.0f, 0.0f, 0}, C{0.0f, 0.0f, 0};
    const int nC = wantC ? nFoot : 0;
    const int nA = v1 ? 128 - __builtin_clzll(v1) : (v0 ? 64 - __builtin_clzll(v0) : 0);  // one past the last visited cell
    // the box is walked row-major (cell t = a * nj + b): column counter and cell offset advance together, no division
    int qcol = 0;
    unsigned cell = __umul24(static_cast<unsigned>(i0), static_cast<unsigned>(cols)) + static_cast<unsigned>(j0);
    const unsigned rowStep = static_cast<unsigned>(cols - nj + 1);
    for (int t0 = 0, c0 = 0; t0 < nA || c0 < nC; t0 += NA, c0 += NC) {
        // bits t0 .. t0 + NA - 1 of the 128-bit membership mask
        const unsigned long long lo = t0 < 64 ? (v0 >> t0) | (t0 ? v1 << (64 - t0) : 0ull) : (t0 < 128 ? v1 >> (t0 - 64) : 0ull);
        const unsigned ba = static_cast<unsigned>(lo) & ((1u << NA) - 1u);
        unsigned bc = 0u;
        float eA[NA], eC[NC];
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            eA[u] = load_cell(elev, ((ba >> u) & 1u) ? cell : 0u);
            const bool wrap = ++qcol == nj;
            qcol = wrap ? 0 : qcol;
            cell += wrap ? rowStep : 1u;
        }
        // eight table entries as two 64-bit words each (the arrays are 16-byte aligned and hold kMaxFootOffsets entries:
        // c0 is a multiple of 8 below nFoot, or 0; entries past nFoot are masked)
        unsigned long long daW, dbW;
        __builtin_memcpy(&daW, da + (c0 < nC ? c0 : 0), 8);
        __builtin_memcpy(&dbW, db + (c0 < nC ? c0 : 0), 8);
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int qi = cRow + static_cast<int8_t>((daW >> (8 * u)) & 0xFFull), qj = cCol + static_cast<int8_t>((dbW >> (8 * u)) & 0xFFull);
            const bool visC = c0 + u < nC && in_range(qi, qj, rows, cols);
            bc |= visC ? (1u << u) : 0u;
            const unsigned cellC = visC ? __umul24(static_cast<unsigned>(qi), static_cast<unsigned>(cols)) + static_cast<unsigned>(qj) : 0u;
            eC[u] = load_cell(elev, cellC);
        }
#pragma unroll
        for (int u = 0; u < NA; ++u) mean_acc(A, ((ba >> u) & 1u) != 0u, eA[u]);
#pragma unroll
        for (int u = 0; u < NC; ++u) mean_acc(C, ((bc >> u) & 1u) != 0u, eC[u]);
    }
    zBox = finish_mean(A.sum, A.last, A.cnt, h);
    zC = finish_mean(C.sum, C.last, C.cnt, h);
}

// The same for a box of up to 32 cells (the generic 8-lane kernels' units), walking the VISITED cells only: a foot disc of
// radius two cells has 13 members in a box of 25 — two batches of eight loads instead of four, i.e. two dependent memory
// round trips less per unit (the register-capped kernel cannot keep more than eight loads in flight: batches of 16 / 25 / 32
// spill and lose, measured).  The members are taken in ascending cell order (lowest set bit first): CircleIterator order.
template <int NA = 8, int NC = 8>
__device__ __forceinline__ void seq_mean2_visited(const float* __restrict__ elev, int rows, int cols, int i0, int j0, int nj, uint32_t vis, bool wantC,
                                                  int cRow, int cCol, const int8_t* da, const int8_t* db, int nFoot, double h, float& zBox, float& zC) {
    static_assert(NC == 8, "the offset table is read eight entries (two 64-bit LDS words) at a time");
    MeanAcc A{0.0f, 0.0f, 0}, C{0.0f, 0.0f, 0};
    const int nC = wantC ? nFoot : 0;
    uint32_t rem = vis;
    const unsigned base = __umul24(static_cast<unsigned>(i0), static_cast<unsigned>(cols)) + static_cast<unsigned>(j0);
    // t / nj for t < 32, 1 <= nj <= 32: floor(t * inv / 2^16) with inv = floor(2^16 / nj) + 1 (error below t / 2^16 < 1 / nj)
    const unsigned inv = static_cast<unsigned>(65536.0f * __builtin_amdgcn_rcpf(static_cast<float>(nj))) + 1u;
    for (int c0 = 0; rem != 0u || c0 < nC; c0 += NC) {
        unsigned ba = 0u, bc = 0u;
        float eA[NA], eC[NC];
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const bool v = rem != 0u;
            const unsigned t = v ? static_cast<unsigned>(__builtin_ctz(rem)) : 0u;
            rem &= rem - 1u;  // (0 stays 0)
            const unsigned a = (t * inv) >> 16, b = t - a * static_cast<unsigned>(nj);
            eA[u] = load_cell(elev, v ? base + __umul24(a, static_cast<unsigned>(cols)) + b : 0u);
            ba |= v ? (1u << u) : 0u;
        }
        unsigned long long daW, dbW;
        __builtin_memcpy(&daW, da + (c0 < nC ? c0 : 0), 8);
        __builtin_memcpy(&dbW, db + (c0 < nC ? c0 : 0), 8);
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int qi = cRow + static_cast<int8_t>((daW >> (8 * u)) & 0xFFull), qj = cCol + static_cast<int8_t>((dbW >> (8 * u)) & 0xFFull);
            const bool visC = c0 + u < nC && in_range(qi, qj, rows, cols);
            bc |= visC ? (1u << u) : 0u;
            const unsigned cellC = visC ? __umul24(static_cast<unsigned>(qi), static_cast<unsigned>(cols)) + static_cast<unsigned>(qj) : 0u;
            eC[u] = load_cell(elev, cellC);
        }
#pragma unroll
        for (int u = 0; u < NA; ++u) mean_acc(A, ((ba >> u) & 1u) != 0u, eA[u]);
#pragma unroll
        for (int u = 0; u < NC; ++u) mean_acc(C, ((bc >> u) & 1u) != 0u, eC[u]);
    }
    zBox = finish_mean(A.sum, A.last, A.cnt, h);
    zC = finish_mean(C.sum, C.last, C.cnt, h);
}

}  // namespace
