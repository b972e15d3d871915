// fpe_margin.hpp — part thirteen of the kernel translation unit (included last in fpe_kernels.hip, behind fpe_trunk.hpp, inside
// namespace fpe): the edge margin (fpe_margin_*, include/fpe.h) — the squared distance, in cells, from a cell to the nearest BAD cell
// within a reach, and the offset that attains it.  Integers only; the planes are the snapshot's tiled bit planes (BitMap).
//
//   The BAD word of (row i, word w) is an OR of the planes C, Df, ~F & in-map and the off-map mask by the call's class bits
//   (margin_bad_word).  A row outside the map, and a word outside its columns, is read from no plane: it is all ones or all zeros by
//   FPE_MARGIN_OFF_MAP alone, so neither the planes' single zero row nor their four zero word groups bound a query's position.
//   margin_row_nearest is the one scan every kernel shares: the 96-bit row w - 1 | w | w + 1 around column j gives two 64-bit windows,
//   one ending and one starting at j (each at least 33 columns), and a leading / trailing zero count gives the nearest BAD bit on
//   either side; the left one wins a tie (lowest dj).  A row's nearest bit is its best under (d2, di, dj), so a cell's answer is the
//   minimum over its rows of the key d2 << 16 | (di + 32) << 8 | (dj + 32) among the rows with d2 <= reach^2.
//
//   margin_map_kernel      dense: a tile of 32 rows x 64 columns per workgroup.  Pass 1: every row of the tile and of a halo of
//                          `reach` rows above and below gets, per column, dj + 32 of its nearest BAD bit (255: none within 31) as a
//                          byte in LDS, one lane per column.  Pass 2: one lane per column of eight cells, 2 reach + 1 byte reads per
//                          cell (consecutive lanes read consecutive bytes), the key minimum, two coalesced stores.
//   margin_cells_kernel<kPlan>   ONE body for the open-loop and the plan-bound form.  2^k lanes per query (4 to 64, chosen from the
//                          reach on the host so that few lane slots idle: margin_lanes_log2), the rows dealt round-robin to the
//                          lanes; xor shuffles inside the group take the key minimum; lane 0 stores the 8-byte record.
//                          kPlan: query s = (b * nCycles + g) * 4 + leg is the cell of nominal[s], when that is valid.
//   margin_summary_kernel  sixteen lanes per pose over its nCycles * 4 records, combined with the reductions of fpe_swing.hpp.
// No atomics, no scratch: every byte is a function of the inputs alone.
#pragma once

namespace {

constexpr int kMarginTileRows = 32, kMarginTileCols = 64;
constexpr int kMarginLdsRows = kMarginTileRows + 2 * FPE_MARGIN_MAX_CELLS;
constexpr uint32_t kMarginNoKey = 0xFFFFFFFFu;
constexpr int kMarginNoDj = 127;  // margin_row_nearest: no BAD bit in the windows

// The BAD bits of the 32 columns of word w in row i; i and w are any integers.
__device__ __forceinline__ uint32_t margin_bad_word(const BitMap& bm, int rows, int cols, int classes, int i, int w) {
    const uint32_t offMap = (classes & FPE_MARGIN_OFF_MAP) ? 0xFFFFFFFFu : 0u;
    if (i < 0 || i >= rows) return offMap;
    const uint32_t in = fmap_col_mask(w, cols);  // 0 for w < 0 and w >= nw
    if (in == 0u) return offMap;
    const uint4 g = bm.words[bit_group_index(i, w, bm.strideW)];
    uint32_t bad = 0u;
    if (classes & FPE_MARGIN_LOW_CANDIDATE) bad |= g.z;
    if (classes & FPE_MARGIN_LOW_DEFAULT) bad |= g.y;
    if (classes & FPE_MARGIN_UNKNOWN) bad |= ~g.w;
    return (bad & in) | (offMap & ~in);
}

// dj of the BAD bit of row i nearest to column j, the left one on a tie; kMarginNoDj when the windows hold none (each window
// spans at least 32 columns beside j: more than FPE_MARGIN_MAX_CELLS).
__device__ __forceinline__ int margin_row_nearest(const BitMap& bm, int rows, int cols, int classes, int i, int j) {
    const int w = j >> 5, b = j & 31;  // (an arithmetic shift: the floor for a negative column too)
    const uint32_t p = margin_bad_word(bm, rows, cols, classes, i, w - 1);
    const uint32_t c = margin_bad_word(bm, rows, cols, classes, i, w);
    const uint32_t n = margin_bad_word(bm, rows, cols, classes, i, w + 1);
    const uint64_t right = ((static_cast<uint64_t>(n) << 32) | c) >> b;        // bit k: column j + k
    const uint64_t left = ((static_cast<uint64_t>(c) << 32) | p) << (31 - b);  // bit 63 - k: column j - k
    const int dr = right ? __builtin_ctzll(right) : 64;
    const int dl = left ? __builtin_clzll(left) : 64;
    if (dl == 64 && dr == 64) return kMarginNoDj;
    return dl <= dr ? -dl : dr;
}

__device__ __forceinline__ uint32_t margin_key(int di, int dj, int reach) {
    const int d2 = di * di + dj * dj;
    return d2 <= reach * reach ? (static_cast<uint32_t>(d2) << 16) | (static_cast<uint32_t>(di + 32) << 8) | static_cast<uint32_t>(dj + 32)
                               : kMarginNoKey;
}

// What the host forms refuse (FPE_E_INVALID_ARG) and the device forms answer with FPE_MARGIN_REFUSED: one function for both
FPE_HD bool margin_cell_refused(int rows, int cols, int row, int col) {
    return row < -FPE_PACKED_BIAS || row >= rows + FPE_PACKED_BIAS || col < -FPE_PACKED_BIAS || col >= cols + FPE_PACKED_BIAS;
}

// The record of a cell from the minimum key of its rows (ids zero)
__device__ __forceinline__ fpe_margin_record margin_record(const MarginConsts& mc, int rows, int cols, int row, int col, uint32_t key) {
    fpe_margin_record rec{};
    uint32_t flags = FPE_MARGIN_FOOTHOLD;
    if (row < 0 || row >= rows || col < 0 || col >= cols) flags |= FPE_MARGIN_CENTRE_OFF_MAP;
    if (key == kMarginNoKey) {
        rec.dist_sq = FPE_MARGIN_NONE;
        flags |= FPE_MARGIN_NO_BAD;
    } else {
        rec.dist_sq = static_cast<uint16_t>(key >> 16);
        rec.di = static_cast<int8_t>(static_cast<int>((key >> 8) & 0xFFu) - 32);
        rec.dj = static_cast<int8_t>(static_cast<int>(key & 0xFFu) - 32);
        if (static_cast<double>(rec.dist_sq) * mc.res2 < mc.minMargin2) flags |= FPE_MARGIN_UNDER;
    }
    rec.flags = static_cast<uint8_t>(flags);
    return rec;
}

__global__ __launch_bounds__(256) void margin_map_kernel(BitMap bm, int rows, int cols, MarginConsts mc, FootmapRoi roi,
                                                         uint16_t* __restrict__ distSq, int8_t* __restrict__ nearest) {
    __shared__ uint8_t rowDj[kMarginLdsRows][kMarginTileCols];
    const int t = static_cast<int>(threadIdx.x);
    const int tx = t & (kMarginTileCols - 1), ty = t >> 6;
    const int reach = mc.reach;
    const int iBase = roi.row0 + static_cast<int>(blockIdx.y) * kMarginTileRows;
    const int j = roi.col0 + static_cast<int>(blockIdx.x) * kMarginTileCols + tx;
    const int nLds = kMarginTileRows + 2 * reach;
    for (int a = ty; a < nLds; a += 4) {
        const int dj = margin_row_nearest(bm, rows, cols, mc.classes, iBase - reach + a, j);
        rowDj[a][tx] = (dj >= -FPE_MARGIN_MAX_CELLS && dj <= FPE_MARGIN_MAX_CELLS) ? static_cast<uint8_t>(dj + 32) : static_cast<uint8_t>(255);
    }
    __syncthreads();
    if (j >= roi.col0 + roi.nc) return;
    for (int u = 0; u < 8; ++u) {
        const int r = ty * 8 + u, i = iBase + r;
        if (i >= roi.row0 + roi.nr) break;
        uint32_t best = kMarginNoKey;
        for (int di = -reach; di <= reach; ++di) {
            const int v = rowDj[r + reach + di][tx];
            if (v != 255) best = min(best, margin_key(di, v - 32, reach));
        }
        const size_t o = static_cast<size_t>(i - roi.row0) * roi.nc + static_cast<size_t>(j - roi.col0);
        const bool none = best == kMarginNoKey;
        if (distSq) distSq[o] = none ? static_cast<uint16_t>(FPE_MARGIN_NONE) : static_cast<uint16_t>(best >> 16);
        if (nearest) {
            nearest[2 * o] = none ? 0 : static_cast<int8_t>(static_cast<int>((best >> 8) & 0xFFu) - 32);
            nearest[2 * o + 1] = none ? 0 : static_cast<int8_t>(static_cast<int>(best & 0xFFu) - 32);
        }
    }
}

// kPlan false: q[n] -> out[n].  kPlan true: n = B * nCycles * 4 records from nominal.  lanesLog2: lanes per query (2..6);
// 256 >> lanesLog2 queries per workgroup.
template <bool kPlan>
__global__ __launch_bounds__(256) void margin_cells_kernel(BitMap bm, int rows, int cols, MarginConsts mc, int lanesLog2,
                                                           const fpe_margin_query* __restrict__ q,
                                                           const fpe_foothold* __restrict__ nominal, int nCycles, int n,
                                                           fpe_margin_record* __restrict__ out) {
    const int t = static_cast<int>(threadIdx.x);
    const int s = static_cast<int>(blockIdx.x) * (256 >> lanesLog2) + (t >> lanesLog2);
    const int lane = t & ((1 << lanesLog2) - 1);
    if (s >= n) return;  // (a whole group at a time: the shuffles stay inside a group)
    int row, col;
    bool live = true;
    if constexpr (kPlan) {
        const fpe_foothold& f = nominal[s];
        row = f.row, col = f.col;
        live = f.valid != 0;
    } else {
        row = q[s].row, col = q[s].col;
    }
    fpe_margin_record rec{};
    if (live) {
        if (margin_cell_refused(rows, cols, row, col)) {
            rec.flags = FPE_MARGIN_REFUSED;
        } else {
            uint32_t key = kMarginNoKey;
            for (int di = lane - mc.reach; di <= mc.reach; di += 1 << lanesLog2) {
                const int dj = margin_row_nearest(bm, rows, cols, mc.classes, row + di, col);
                if (dj != kMarginNoDj) key = min(key, margin_key(di, dj, mc.reach));
            }
            for (int o = (1 << lanesLog2) >> 1; o > 0; o >>= 1) key = min(key, static_cast<uint32_t>(__shfl_xor(static_cast<int>(key), o)));
            rec = margin_record(mc, rows, cols, row, col, key);
        }
    }
    if constexpr (kPlan) {
        rec.foot_id = static_cast<uint8_t>(s & 3);
        rec.gait_cycle_id = static_cast<uint8_t>((s >> 2) % nCycles);
    }
    if (lane == 0) out[s] = rec;
}

// Sixteen lanes per pose over its nCycles * 4 records (include/fpe.h: fpe_margin_summary)
__global__ __launch_bounds__(256, 8) void margin_summary_kernel(const fpe_margin_record* __restrict__ records, int B, int nCycles,
                                                                fpe_margin_summary* __restrict__ summary) {
    const int b = static_cast<int>(blockIdx.x) * kSwingPerBlock + static_cast<int>(threadIdx.x) / kSwingLanes;
    const int lane = static_cast<int>(threadIdx.x) & (kSwingLanes - 1);
    if (b >= B) return;
    const int nRec = nCycles * 4;
    const fpe_margin_record* __restrict__ rec = records + static_cast<size_t>(b) * nRec;
    unsigned long long best = ~0ull;  // dist_sq << 16 | g * 4 + leg: the lowest (dist_sq, g, leg)
    int nFoot = 0, nUnder = 0, nOff = 0, firstUnder = 255;
    for (int k = lane; k < nRec; k += kSwingLanes) {
        const uint32_t f = rec[k].flags;
        if (!(f & FPE_MARGIN_FOOTHOLD)) continue;
        ++nFoot;
        const unsigned long long key = (static_cast<unsigned long long>(rec[k].dist_sq) << 16) | static_cast<unsigned long long>(k);
        best = key < best ? key : best;
        if (f & FPE_MARGIN_UNDER) {
            ++nUnder;
            firstUnder = min(firstUnder, k >> 2);
        }
        if (f & FPE_MARGIN_CENTRE_OFF_MAP) ++nOff;
    }
    best = swing_min64u(best);
    nFoot = swing_sum32(nFoot);
    nUnder = swing_sum32(nUnder);
    nOff = swing_sum32(nOff);
    firstUnder = swing_min32(firstUnder);
    if (lane != 0) return;
    fpe_margin_summary s{};
    const int k = static_cast<int>(best & 0xFFFFull);
    s.min_dist_sq = nFoot > 0 ? static_cast<uint16_t>(best >> 16) : static_cast<uint16_t>(FPE_MARGIN_NONE);
    s.min_cycle = nFoot > 0 ? static_cast<uint8_t>(k >> 2) : static_cast<uint8_t>(255);
    s.min_leg = nFoot > 0 ? static_cast<uint8_t>(k & 3) : static_cast<uint8_t>(255);
    s.n_footholds = static_cast<uint16_t>(nFoot);
    s.n_under = static_cast<uint16_t>(nUnder);
    s.n_off_map = static_cast<uint16_t>(nOff);
    s.first_under_cycle = static_cast<uint8_t>(firstUnder);
    summary[b] = s;
}

}  // namespace

bool margin_query_refused(int rows, int cols, const fpe_margin_query& q) { return margin_cell_refused(rows, cols, q.row, q.col); }

// Lanes per query, 2^k with k = 2..6.  A group of L lanes takes the 2 reach + 1 rows in ceil(rows / L) rounds, so a query costs
// L * rounds lane slots; the choice is the L with the fewest slots among those of at most eight rounds, the larger L on a tie
// (fewer rounds): 4 lanes and 5 rounds at the default reach 8 (20 slots for 17 rows, sixteen queries per wavefront), 64 lanes at 31.
int margin_lanes_log2(int reach) {
    const int nRows = 2 * reach + 1;
    int best = 6, bestSlots = 1 << 30;
    for (int k = 6; k >= 2; --k) {
        const int rounds = (nRows + (1 << k) - 1) >> k;
        if (rounds <= 8 && (rounds << k) < bestSlots) best = k, bestSlots = rounds << k;
    }
    return best;
}

hipError_t launch_margin_map(const BitMap& bm, const MapGeom& g, const MarginConsts& mc, const FootmapRoi& roi, uint16_t* d_distSq,
                             int8_t* d_nearest, hipStream_t stream) {
    const dim3 grid((roi.nc + kMarginTileCols - 1) / kMarginTileCols, (roi.nr + kMarginTileRows - 1) / kMarginTileRows);
    hipLaunchKernelGGL(margin_map_kernel, grid, dim3(256), 0, stream, bm, g.rows, g.cols, mc, roi, d_distSq, d_nearest);
    return hipGetLastError();
}

hipError_t launch_margin_cells(const BitMap& bm, const MapGeom& g, const MarginConsts& mc, const fpe_margin_query* d_q, int n,
                               fpe_margin_record* d_out, hipStream_t stream) {
    const int k = margin_lanes_log2(mc.reach), per = 256 >> k;
    hipLaunchKernelGGL(margin_cells_kernel<false>, dim3((n + per - 1) / per), dim3(256), 0, stream, bm, g.rows, g.cols, mc, k, d_q,
                       static_cast<const fpe_foothold*>(nullptr), 1, n, d_out);
    return hipGetLastError();
}

// d_records: B * nCycles * 4 records (required: the summary reads them); d_summary: B elements, or null
hipError_t launch_margin_plan(const BitMap& bm, const MapGeom& g, const MarginConsts& mc, const fpe_foothold* d_nominal, int B, int nCycles,
                              fpe_margin_record* d_records, fpe_margin_summary* d_summary, hipStream_t stream) {
    const int n = B * nCycles * 4;
    const int k = margin_lanes_log2(mc.reach), per = 256 >> k;
    hipLaunchKernelGGL(margin_cells_kernel<true>, dim3((n + per - 1) / per), dim3(256), 0, stream, bm, g.rows, g.cols, mc, k,
                       static_cast<const fpe_margin_query*>(nullptr), d_nominal, nCycles, n, d_records);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !d_summary) return e;
    hipLaunchKernelGGL(margin_summary_kernel, dim3((B + kSwingPerBlock - 1) / kSwingPerBlock), dim3(256), 0, stream, d_records, B, nCycles,
                       d_summary);
    return hipGetLastError();
}
