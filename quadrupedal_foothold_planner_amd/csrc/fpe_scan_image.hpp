// fpe_scan_image.hpp — part nineteen of the kernel translation unit (included at the end of fpe_kernels.hip, inside namespace fpe,
// behind fpe_scan.hpp, fpe_scan_clear.hpp and fpe_scan_close.hpp, whose constants, helpers and kernels it uses): the image forms of
// the scan entry points (fpe_scan_*_image*; include/fpe.h, point 6 of the scan block).  A depth or range image is fused and cleared
// without a point cloud: a pixel becomes its three floats in registers, by the contract's f32 rule, and goes straight into
// scan_classify / clear_ray_of.  No kernel here writes an x, y, z triple to memory.
//
//   scan_image_point         the three floats of point ordinal i: the selected pixel (ri, ci) = (i / selCols, i % selCols), its element at
//                            (ri * rowStep) * pitch + ci * colStep (a 2-byte or a 4-byte load; with colStep 1 a wavefront's 64 pixels
//                            are one 128- or 256-byte run), the depth in metres, then the pinhole or the spherical rule.  Every
//                            operation is f32 and rounded on its own (the build's -ffp-contract=off), the divisions are IEEE divisions.
//                            An invalid pixel is (NaN, NaN, NaN): the fuse's test 1 drops it.
//   scan_top_image_kernel    scan_top_kernel<merge = true> with that source: one lane per selected pixel, the 8-byte record, runs of
//                            equal cells reduced in registers, one atomicMax per run.  The five class counts are summed per workgroup
//                            in LDS (one LDS atomic per wavefront and non-zero class) and leave as ONE global atomic per workgroup and
//                            non-zero class, into the accumulator words 1-5 that scan_fuse_kernel's last workgroup collects.
//   ClearImageSource         the ray kernels' point source (fpe_scan_clear.hpp): both forms of the ray pass, at every group width.
// scan_sum_kernel<true>, scan_fuse_kernel and scan_clear_cells_kernel run unchanged behind these.  No float atomics.
#pragma once

namespace {

__device__ __forceinline__ void scan_image_point(const ScanImage& im, int i, float& x, float& y, float& z) {
    const int ri = i / im.selCols;
    const int ci = i - ri * im.selCols;
    const int v = ri * im.rowStep, u = ci * im.colStep;
    const size_t k = static_cast<size_t>(v) * static_cast<size_t>(im.pitch) + static_cast<size_t>(u);
    float d;
    bool valid;
    if (im.format == FPE_SCAN_DEPTH_U16) {
        const uint16_t raw = static_cast<const uint16_t*>(im.data)[k];
        valid = raw != 0;
        d = static_cast<float>(raw) * im.scale;
    } else {
        const float raw = static_cast<const float*>(im.data)[k];
        valid = __builtin_isfinite(raw) && raw > 0.0f;
        d = raw * im.scale;
    }
    if (!valid) {
        x = y = z = __uint_as_float(kScanCleared);
        return;
    }
    if (im.model == FPE_SCAN_IMAGE_PINHOLE) {
        x = ((static_cast<float>(u) - im.cx) * d) / im.fx;
        y = ((static_cast<float>(v) - im.cy) * d) / im.fy;
        z = d;
    } else {
        const float ce = im.rowDir[2 * v], se = im.rowDir[2 * v + 1];  // (a caller's table is only float-aligned: two loads each)
        const float ca = im.colDir[2 * u], sa = im.colDir[2 * u + 1];
        const float w = d * ce;
        x = w * ca;
        y = w * sa;
        z = d * se;
    }
}

__global__ __launch_bounds__(kScanBlock) void scan_top_image_kernel(ScanArgs a) {
    __shared__ int32_t sCnt[5];
    if (threadIdx.x < 5) sCnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int i = static_cast<int>(blockIdx.x) * kScanBlock + static_cast<int>(threadIdx.x);
    ScanPoint p{5, kScanNoCell, 0};  // (5: a lane behind the last point)
    if (i < a.n) {
        float x, y, z;
        scan_image_point(a.im, i, x, y, z);
        p = scan_classify(a, x, y, z);
        a.rec[i] = make_uint2(p.cell, static_cast<uint32_t>(p.q));
    }
    // the wavefront's class counts into LDS: one LDS atomic per wavefront and non-zero class
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const unsigned long long m = __ballot(p.cls == c);
        if (lane == 0 && m != 0ull) atomicAdd(sCnt + c, static_cast<int32_t>(__popcll(m)));
    }
    // the merged maximum (scan_top_kernel<true>'s): one atomicMax per run of equal cells
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
    // one global atomic per workgroup and non-zero class
    __syncthreads();
    if (threadIdx.x < 5 && sCnt[threadIdx.x] != 0) atomicAdd(a.acc + 1 + threadIdx.x, sCnt[threadIdx.x]);
}

struct ClearImageSource {
    static __device__ __forceinline__ void xyz(const ScanClearArgs& a, int i, float& x, float& y, float& z) { scan_image_point(a.im, i, x, y, z); }
};

}  // namespace

hipError_t launch_scan_top_image(const ScanArgs& a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scan_top_image_kernel, dim3(scan_blocks(static_cast<size_t>(a.n))), dim3(kScanBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_scan_fuse_image(const ScanArgs& a, hipStream_t stream) {
    hipError_t e = launch_scan_top_image(a, stream);
    if (e == hipSuccess) e = launch_scan_sum(a, true, stream);
    if (e == hipSuccess) e = launch_scan_cells(a, stream);
    return e;
}

hipError_t launch_scan_clear_image(const ScanClearArgs& a, int form, int group, hipStream_t stream) {
    hipError_t e = clear_rays_launch<ClearImageSource>(a, form, group, stream);
    if (e == hipSuccess) e = launch_scan_clear_cells(a, stream);
    return e;
}
