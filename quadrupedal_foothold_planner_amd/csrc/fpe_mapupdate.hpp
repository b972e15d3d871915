// fpe_mapupdate.hpp — part ten of the kernel translation unit (included at the end of fpe_kernels.hip, inside namespace fpe):
// incremental map updates (fpe_update_map*, include/fpe.h).
//
// The new snapshot is the base snapshot shifted by whole cells, the cells that have no source filled with grid_map's cleared
// value, and a few rectangles written over that.  Snapshots are canonical and the bit planes are per-cell predicates, so this is
// ONE streaming pass: every destination cell selects its source, both layers are stored, and the planes of every carried
// threshold pair are balloted from the traversability values while they pass through — not shifted from the old plane words
// (a shift by (sr, sc) would cut across the 8-row x 32-column plane lines in both axes).
//
//   map_update_kernel   a workgroup owns one ROW GROUP of the planes (8 consecutive rows r1 = i + 1 in [8 g, 8 g + 8): rows
//                       8 g - 1 .. 8 g + 6) x 256 columns, a wavefront 8 rows x 64 columns, lane = column.  Every wavefront
//                       instruction reads or writes 64 consecutive floats of one row (256 bytes; the shifted source rows start
//                       sc floats off the destination's alignment and stay whole-line runs), sixteen loads in flight per thread
//                       before the first store.  Patches are tested against the wavefront's 8 x 64 cells with scalar compares,
//                       so a wavefront no patch touches runs none of the per-cell patch code; one that is touched reads the
//                       patch element by its two strides (row- or column-major: the reads are small).  Planes: a row's four
//                       ballots (canon_plane_row's predicates) cover two 32-column words; with the 8 rows of the group in
//                       registers, lanes 0-15 pick row (lane & 7) of word (lane >> 3) and the wavefront stores 16 consecutive
//                       uint4 — its two whole 128-byte plane lines (bit_group_index: 8 rows x one word) — in one instruction
//                       per pair.  Rows -1 and `rows` of the planes fall into a group as rows of zeros; the padding word
//                       groups are zeroed by launch_map_update, as launch_canonicalise does.
// Values travel as 32-bit patterns.
// fpe_update_elevation* (the producer's filters on the dirty region only) runs the same kernel with elevation-only patches — a patch
// with a null traversability pointer leaves the carried or cleared value — and with no pairs: the chain writes the traversability
// behind this pass, and the planes are built from the finished layer.
#pragma once

namespace {

constexpr uint32_t kUpdateCleared = 0x7FC00000u;  // the quiet NaN of a cell grid_map::move has cleared
constexpr int kUpdateRows = 8;                    // rows of a plane line
constexpr int kUpdateCols = 256;                  // columns of a workgroup

__global__ __launch_bounds__(256) void map_update_kernel(MapUpdateArgs a) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int jWave = static_cast<int>(blockIdx.x) * kUpdateCols + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) & ~63);
    const int j = jWave + lane;
    const int g = static_cast<int>(blockIdx.y);
    const int iFirst = kUpdateRows * g - 1;  // the group's first row (row -1 of the planes in group 0)
    const int rows = a.rows, cols = a.cols;

    uint32_t t[kUpdateRows], e[kUpdateRows];
    const int sj = j + a.sc;
    const bool colCarried = j < cols && sj >= 0 && sj < cols;
#pragma unroll
    for (int r = 0; r < kUpdateRows; ++r) {
        const int i = iFirst + r, si = i + a.sr;
        t[r] = kUpdateCleared;
        e[r] = kUpdateCleared;
        if (colCarried && i >= 0 && i < rows && si >= 0 && si < rows) {
            const size_t k = static_cast<size_t>(si) * cols + sj;
            t[r] = a.baseTrav[k];
            e[r] = a.baseElev[k];
        }
    }
    for (int p = 0; p < a.nPatches; ++p) {  // in order: the later patch wins
        const MapUpdatePatch& q = a.patch[p];
        // (scalar: the wavefront's 8 x 64 cells against the rectangle)
        if (iFirst + kUpdateRows <= q.row0 || iFirst >= q.row0 + q.nr || jWave + 64 <= q.col0 || jWave >= q.col0 + q.nc) continue;
        const int pj = j - q.col0;
        if (pj < 0 || pj >= q.nc) continue;
#pragma unroll
        for (int r = 0; r < kUpdateRows; ++r) {
            const int pi = iFirst + r - q.row0;
            if (pi >= 0 && pi < q.nr) {
                const int64_t k = pi * q.rowStride + pj * q.colStride;
                if (q.trav) t[r] = q.trav[k];  // (null: the elevation-only form of fpe_update_elevation* — the carried or cleared value stays)
                e[r] = q.elev[k];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kUpdateRows; ++r) {
        const int i = iFirst + r;
        if (j < cols && i >= 0 && i < rows) {
            const size_t k = static_cast<size_t>(i) * cols + j;
            a.dstTrav[k] = t[r];
            a.dstElev[k] = e[r];
        }
    }
    const int w = jWave / 32 + (lane >> 3);  // lanes 0-15: word (lane >> 3) of the wavefront's two, row (lane & 7) of the group
    const int sh = 32 * ((lane >> 3) & 1);
    for (int p = 0; p < a.nPairs; ++p) {
        const float thrD = a.pair[p].thrD, thrC = a.pair[p].thrC;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int r = 0; r < kUpdateRows; ++r) {
            const int i = iFirst + r;
            const float v = __uint_as_float(t[r]);
            const bool in = j < cols && i >= 0 && i < rows;
            const bool fin = in && __builtin_isfinite(v);
            const bool d = in && v < thrD;  // raw compare: NaN -> false, -inf -> true (canon_plane_row)
            const bool c = fin && v < thrC;
            const unsigned long long bD = __ballot(d), bDf = __ballot(d && fin), bC = __ballot(c), bF = __ballot(fin);
            if ((lane & 7) == r) {
                o.x = static_cast<unsigned>(bD >> sh);
                o.y = static_cast<unsigned>(bDf >> sh);
                o.z = static_cast<unsigned>(bC >> sh);
                o.w = static_cast<unsigned>(bF >> sh);
            }        }
        // (group g's rows are r1 = 8 g + r: bit_group_index(iFirst + r, w, strideW) with r = lane & 7)
        if (lane < 16 && w < a.nw)
            a.pair[p].words[((static_cast<size_t>(g) * a.strideW + static_cast<size_t>(w + kBitPadW)) << 3) + static_cast<size_t>(lane & 7)] = o;
    }
}

}  // namespace

// One update on `stream`: the plane buffers zeroed first (padding word groups; recycled buffers are dirty), then one launch.
// The engine has validated the patches (inside the map, one of the two stride forms) and clamped the shift.
hipError_t launch_map_update(const MapUpdateArgs& a, hipStream_t stream) {
    MapUpdateArgs k = a;
    const size_t units = bitmap_words(a.rows, a.cols, &k.strideW, &k.nw);
    for (int p = 0; p < a.nPairs; ++p) {
        const hipError_t e = hipMemsetAsync(a.pair[p].words, 0, units * 4, stream);
        if (e != hipSuccess) return e;
    }
    dim3 grid((a.cols + kUpdateCols - 1) / kUpdateCols, bit_row_groups(a.rows));
    hipLaunchKernelGGL(map_update_kernel, grid, dim3(256), 0, stream, k);
    return hipGetLastError();
}
