// fpe_layers.hpp — part eight of the kernel translation unit (included at the end of fpe_kernels.hip, inside namespace fpe):
// the dense maps as grid_map message layers (fpe_export_layers*, include/fpe.h).
//
// The mirror image of canonicalise_layer_kernel: that kernel turns a message layer (column-major, rotated by the circular
// buffer's start index) into the canonical one (row-major, start index (0,0)); this one turns the canonical PRODUCTS of the dense
// calls — uint8 flags and codes, interleaved int8 offset pairs, f32 heights, all covering the region only — into message layers:
// f32 of the whole map, NaN outside the region, in the destination's storage order and rotated by its start index.
//
//   layers_export_kernel   one launch for every layer of a call: blockIdx.z names the slot of the layer table in the argument
//                          block, blockIdx.x / .y a 64 x 64 tile of the WHOLE map in canonical indices.  A wavefront reads 64
//                          consecutive cells of one canonical row (the sources are row-major: coalesced; only cells inside the
//                          region are read, every other cell is the NaN pattern) with sixteen loads in flight per thread.
//                          Row-major destinations are stored as read, a wavefront per wrapped row.  Column-major destinations go
//                          through the [64][65] LDS transpose, so that a wavefront store covers 64 consecutive floats of one
//                          buffer column.  The wrap by (si, sj) is applied per element — it may fall inside a tile.  Where the
//                          host proved it (column-major, rows % 4 == 0, si % 4 == 0, every destination 16-byte aligned: a group
//                          of four consecutive canonical rows then neither straddles the wrap nor the end of a column and starts
//                          aligned) four rows leave in one 16-byte store, as on canonicalise_layer_kernel's cols % 4 path.
// Values travel as 32-bit patterns (the f32 products bit for bit); the conversions uint8 -> float and int8 -> float are exact.
#pragma once

namespace {

constexpr int kLayersTile = 64;
constexpr uint32_t kLayersNoData = 0x7FC00000u;  // the quiet NaN grid_map reads as "no data"

// The 32-bit pattern of the layer's float for element `idx` of its canonical product
template <int kKind>
__device__ __forceinline__ uint32_t layer_value(const void* __restrict__ src, size_t idx) {
    if constexpr (kKind == kLayerSrcU8) {
        return __float_as_uint(static_cast<float>(static_cast<const uint8_t*>(src)[idx]));
    } else if constexpr (kKind == kLayerSrcF32) {
        return static_cast<const uint32_t*>(src)[idx];
    } else {
        return __float_as_uint(static_cast<float>(static_cast<const int8_t*>(src)[2 * idx + (kKind == kLayerSrcI8Pair1 ? 1 : 0)]));
    }
}

// One tile of one layer.  t: the transpose tile (column-major destinations only)
template <int kKind>
__device__ __forceinline__ void layers_tile(const LayersArgs& a, const void* __restrict__ src, uint32_t* __restrict__ dst,
                                            uint32_t (&t)[kLayersTile][kLayersTile + 1]) {
    constexpr int T = kLayersTile, kPer = T * T / 256, kStep = 256 / T;
    const int tx = threadIdx.x & (T - 1), ty = threadIdx.x / T;
    const int iBase = blockIdx.y * T, jBase = blockIdx.x * T;
    const int rows = a.rows, cols = a.cols;
    // canonical rows: consecutive threads walk j (contiguous in the source)
    uint32_t v[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int r = iBase + ty + kStep * q - a.roi.row0, c = jBase + tx - a.roi.col0;
        v[q] = kLayersNoData;
        if (r >= 0 && r < a.roi.nr && c >= 0 && c < a.roi.nc) v[q] = layer_value<kKind>(src, static_cast<size_t>(r) * a.roi.nc + c);
    }
    if (a.dstRowMajor) {
        int bj = jBase + tx + a.sj;
        if (bj >= cols) bj -= cols;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int i = iBase + ty + kStep * q;
            if (i < rows && jBase + tx < cols) {
                int bi = i + a.si;
                if (bi >= rows) bi -= rows;
                dst[static_cast<size_t>(bi) * cols + bj] = v[q];
            }
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) t[ty + kStep * q][tx] = v[q];  // t[row][column] of the tile
    __syncthreads();
    if (a.vec16) {  // four canonical rows per thread, one 16-byte store (see the head of this file for when)
        constexpr int kGroups = T / 4, kColsPerPass = 256 / kGroups;
        const int g4 = threadIdx.x % kGroups, c0 = threadIdx.x / kGroups;
#pragma unroll
        for (int q = 0; q < T / kColsPerPass; ++q) {
            const int c = c0 + kColsPerPass * q, i = iBase + 4 * g4, j = jBase + c;
            if (i < rows && j < cols) {  // (rows % 4 == 0: i + 3 < rows as well)
                int bi = i + a.si;
                if (bi >= rows) bi -= rows;
                int bj = j + a.sj;
                if (bj >= cols) bj -= cols;
                uint4 o;
                o.x = t[4 * g4 + 0][c]; o.y = t[4 * g4 + 1][c]; o.z = t[4 * g4 + 2][c]; o.w = t[4 * g4 + 3][c];
                *reinterpret_cast<uint4*>(dst + static_cast<size_t>(bj) * rows + bi) = o;
            }
        }
        return;
    }
    // consecutive threads walk i (contiguous in a buffer column, up to the wrap)
    int bi = iBase + tx + a.si;
    if (bi >= rows) bi -= rows;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int j = jBase + ty + kStep * q;
        if (iBase + tx < rows && j < cols) {
            int bj = j + a.sj;
            if (bj >= cols) bj -= cols;
            dst[static_cast<size_t>(bj) * rows + bi] = t[tx][ty + kStep * q];
        }
    }
}

__global__ __launch_bounds__(256) void layers_export_kernel(LayersArgs a) {
    __shared__ uint32_t t[kLayersTile][kLayersTile + 1];
    const LayerSlot s = a.slot[blockIdx.z];
    uint32_t* dst = reinterpret_cast<uint32_t*>(s.dst);
    switch (s.kind) {  // (uniform over the workgroup)
        case kLayerSrcU8: layers_tile<kLayerSrcU8>(a, s.src, dst, t); break;
        case kLayerSrcI8Pair0: layers_tile<kLayerSrcI8Pair0>(a, s.src, dst, t); break;
        case kLayerSrcI8Pair1: layers_tile<kLayerSrcI8Pair1>(a, s.src, dst, t); break;
        default: layers_tile<kLayerSrcF32>(a, s.src, dst, t); break;
    }
}

}  // namespace

// The layers of `a` (validated by the engine: 1 <= nLayers <= FPE_LAYER_COUNT, start index inside the map, region inside the
// map, every pointer set) on `stream`, one launch.
hipError_t launch_layers_export(const LayersArgs& a, hipStream_t stream) {
    LayersArgs k = a;
    bool vec = !a.dstRowMajor && (a.rows & 3) == 0 && (a.si & 3) == 0;
    for (int l = 0; l < a.nLayers; ++l) vec = vec && (reinterpret_cast<uintptr_t>(a.slot[l].dst) & 15u) == 0;
    k.vec16 = vec ? 1 : 0;
    dim3 grid((a.cols + kLayersTile - 1) / kLayersTile, (a.rows + kLayersTile - 1) / kLayersTile, a.nLayers);
    hipLaunchKernelGGL(layers_export_kernel, grid, dim3(256), 0, stream, k);
    return hipGetLastError();
}
