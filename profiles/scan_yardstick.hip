// The streaming yardstick of profiles/probe_scan.py: one lane per point reads the point's three floats (the stride scan_top_kernel
// reads them with) and writes eight bytes — the traffic of the scan fusion's first pass without its arithmetic and without an atomic.
// Built by profiles/collect_scan.sh into profiles/_build/libscan_yardstick.so; not part of the engine.
#include <hip/hip_runtime.h>
#include <cstdint>

__global__ __launch_bounds__(256) void scan_stream_kernel(const float* points, int stride, int n, uint2* out) {
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (i >= n) return;
    const float* s = points + static_cast<size_t>(i) * static_cast<size_t>(stride);
    out[i] = make_uint2(__float_as_uint(s[0]) ^ __float_as_uint(s[1]), __float_as_uint(s[2]));
}

extern "C" int scan_yardstick(const float* points, int stride, int n, void* out, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(scan_stream_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), points, stride, n, static_cast<uint2*>(out));
    return static_cast<int>(hipGetLastError());
}
