// fpe_bits.hpp — part two of the kernel translation unit (included at the end of fpe_kernels.hip, inside
// namespace fpe): the BIT-WINDOW kernels.
//
// Per map snapshot and threshold pair the engine keeps four bit planes (BitMap, fpe_device.hpp): D (trav <
// defaultFootholdThreshold_, raw compare), Df (the same for finite cells only), C (finite && trav <
// candidateFootholdThreshold_), F (finite).  A leg's search window — every cell its default disc, centroid
// rectangle (cpp:1615-1750) and spiral candidates' foot discs (cpp:2085-2163) can touch — is then one 32-bit row
// mask per plane and window row: lane s of the leg's group loads rows s, s + G, ... (two 16-byte loads per row),
// and everything the reference decides by comparing traversability values becomes bit arithmetic:
//   * centroid row scan (cpp:1717-1750): popcount of the D row under the rectangle's column mask;
//   * checkDefaultFoothold (cpp:2039-2082): Df bit of every cell of the disc (membership stays the f64 test);
//   * checkCirclePolygonFoothold (cpp:2117-2163) for EVERY candidate at once: per window row
//         P = ~F | (~C & inside)      ("cell does not fail": non-finite, or above threshold and inside the polygon)
//     eroded with the host-proved foot-disc offset table, E = AND_k shift(P[row + da_k], db_k); a candidate is
//     valid iff its E bit is set, so a spiral round is an LDS read and a bit test — no map access at all.
//     The reference rectangle's PNPOLY test is exact in INDEX space: cell centres are monotone in the index, so
//     {i : xlo <= x_i < xhi} is an index interval whose ends are found by evaluating the reference's own f64
//     comparison at the two indices next to a predicted boundary.  Other polygons keep the per-cell PNPOLY test,
//     applied only to candidates that pass the threshold erosion.
// The f32 elevation layer is read for the mean heights only (cpp:2520-2554, unchanged ordered sums).
// Exactness rests on three host-side proofs (bits_supported): the foot-disc offset table (derive_foot_offsets), the
// window half-width (every cell that can be touched lies inside it), and getIndex(submap cell centre) == top-left +
// (row, col) for the centroid result.  When a proof fails the engine launches the direct kernels instead.
#pragma once

// ---- products as a compile-time mask --------------------------------------------------------------------------------
// Which of fpe_plan_out's products a launch writes is a run-time null test per product in the generic instantiation
// (kProd = 0: any combination).  The two shapes that matter are compiled on their own: kProd = 2, ALL seven base products
// (bench.py's headline step, fpe_plan with every array: the tests fold away) and kProd = 1, the NOMINAL track only —
// {nominal, selected, selected_packed, cycle_ok}: the service's response (cpp:1588) and the multi-GPU exchange record —
// where the default-track disc (its loads, membership, deposits and height sums), the centroid result's height and record,
// the stance and the first-cycle gate are not compiled at all.  The engine picks the instantiation from the pointers.
template <int kProd>
__device__ __forceinline__ fpe_plan_out specialise_products(fpe_plan_out out) {
    if constexpr (kProd == 1) {
        out.centroid = nullptr;
        out.default_next = nullptr;
        out.stance = nullptr;
        out.pose_status = nullptr;
    } else if constexpr (kProd == 2) {
        __builtin_assume(out.nominal != nullptr);
        __builtin_assume(out.centroid != nullptr);
        __builtin_assume(out.default_next != nullptr);
        __builtin_assume(out.cycle_ok != nullptr);
        __builtin_assume(out.stance != nullptr);
        __builtin_assume(out.selected != nullptr);
        __builtin_assume(out.pose_status != nullptr);
    }
    return out;
}
__host__ inline int product_shape(const fpe_plan_out& o) {
    if (o.nominal && o.centroid && o.default_next && o.cycle_ok && o.stance && o.selected && o.pose_status) return 2;
    if (!o.centroid && !o.default_next && !o.stance && !o.pose_status) return 1;
    return 0;
}

// ---- the device code, by kernel family ------------------------------------------------------------------------------
// Pieces of this translation unit like this file itself (inside namespace fpe, not stand-alone; each opens and closes the
// anonymous namespace for its helpers), in the order that keeps the kernels' order in the code object.  build.py lists
// them: a piece missing there would let a stale library count as up to date.
#include "fpe_bits_window.hpp"  // what both families use: planes, window rows, centroid scan, erosion, spiral_bits, seq_mean2
#include "fpe_bits_lane8.hpp"   // 8 lanes per leg: plan_bits_kernel
#include "fpe_bits_seq.hpp"     // one wavefront per pose: plan_bits_seq_kernel

// ---- host side of the bit-window path --------------------------------------------------------------------------
size_t bitmap_words(int rows, int cols, int* strideW, int* nw) {
    *nw = (cols + 31) / 32;
    *strideW = *nw + 2 * kBitPadW;
    return static_cast<size_t>(bit_row_groups(rows)) * 8 * (*strideW) * 4;  // 4-byte units (4 planes per word group, 8 rows per tile)
}

hipError_t launch_build_bitmap(const float* d_trav, int rows, int cols, float thrDefault, float thrCandidate, uint32_t* d_words,
                               hipStream_t stream) {
    int strideW, nw;
    const size_t units = bitmap_words(rows, cols, &strideW, &nw);
    hipError_t e = hipMemsetAsync(d_words, 0, units * 4, stream);  // padding rows / word groups; recycled buffers are dirty
    if (e != hipSuccess) return e;
    dim3 grid((cols + 255) / 256, rows);
    hipLaunchKernelGGL(build_bitmap_kernel, grid, dim3(256), 0, stream, d_trav, rows, cols, thrDefault, thrCandidate,
                       reinterpret_cast<uint4*>(d_words), strideW, nw);
    return hipGetLastError();
}

// Kernel shape for a window half-width: 8 lanes per leg with 2-4 rows per lane (windows of up to 32 rows / columns);
// one wavefront per pose with 64-bit rows (up to 64 rows) or 96-bit rows (up to 96 columns, 2 rows per lane).
// (Which instantiation a call launches, and the launch itself: select_plan_kernel / launch_plan, fpe_plan_launch.hpp.)
struct BitsShape {
    int lanes;  // 8 or 64; 0 = no instantiation fits
    int nrl, kw;
};
static BitsShape bits_shape(int winH) {
    const int side = 2 * winH + 1;
    if (winH <= 0) return {0, 0, 0};
    if (side <= 16) return {8, 2, 1};
    if (side <= 24) return {8, 3, 1};
    if (side <= 32) return {8, 4, 1};
    if (side <= 64) return {64, 1, 2};
    if (side <= 96) return {64, 2, 3};
    return {0, 0, 0};
}

bool bits_supported(const PlanConsts& pc, const MapGeom& g) {
    if (pc.noBits != 0 || pc.winH <= 0) return false;
    // 32-bit offsets into layers and planes (load_cell / load_group), 24-bit multiplies of rows and strides
    if (g.rows >= (1 << 24) - 2 || g.cols >= (1 << 24) - 64) return false;
    if (static_cast<double>(g.rows) * g.cols * 4.0 >= 2147483648.0 - 65536.0) return false;
    if ((static_cast<double>(g.rows) + 16.0) * ((g.cols + 31) / 32 + 2 * kBitPadW) * 16.0 >= 2147483648.0) return false;
    const BitsShape sp = bits_shape(pc.winH);
    if (sp.lanes == 0) return false;
    if (pc.groupOverride != 0 && pc.groupOverride != (sp.lanes == 8 ? 8 : 65)) return false;
    if (pc.nFoot > (sp.lanes == 8 ? kDiscRounds * 8 : 64)) return false;  // the offset table is walked one entry per lane
    // the per-leg LDS (3 row arrays) doubles as float scratch of a direct disc pass over a CircleIterator
    // bounding box of up to (2 ceil(rf / res) + 2)^2 cells
    const double side = 2.0 * ceil(pc.rf / g.res) + 2.0;
    if (sp.lanes == 64) return side * side <= kBitsMaxBoxCells;  // 64-lane kernels: membership in two rounds of 64 cells (SeqRec::visA / visB)
    return side * side <= legbits_words(8 * sp.nrl, 1, pc.nHW);
}
