// fpe_scan_clear.hpp — part seventeen of the kernel translation unit (included at the end of fpe_kernels.hip, inside namespace fpe,
// behind fpe_scan.hpp whose constants and helpers it uses): scan visibility clearing (fpe_scan_clear*, include/fpe.h): the cells of a
// state that the rays of a new scan pass below become unknown.
//
// The prior is read by the ray pass and written by the cell pass only, and the one per-cell reduction is an integer count (the hits,
// in ScanCell's `count` word: 0 at rest), so the result does not depend on the order of the points or of the atomics.  Two launches:
//
//   ray pass     every point that casts a ray (i % ray_stride == 0) is classified by the fuse's tests 1-4; a ray's samples
//                k = start .. K - end - 1 are placed by the contract's rule in f64 (t = k / K by a true division, each product and sum
//                rounded on its own).  x and y are monotone in k, so the samples of a ray that fall into one cell are consecutive: a
//                RUN.  A run with at least one violating sample issues ONE atomicAdd on the cell's hits.  Two forms, same results, each
//                with the point source as a template parameter (ClearPointSource here: the call's points; fpe_scan_image.hpp's
//                ClearImageSource: a pixel); clear_ray_of is everything from the point where a ray has its x, y, z:
//       scan_clear_rays_lane_kernel      one lane per ray, looping over its samples; the current cell and a violated flag in
//                                        registers, the atomic when the cell changes.
//       scan_clear_rays_group_kernel<G>  G = 16, 32 or 64 adjacent lanes per ray, a chunk of G samples per step.  Runs are found as
//                                        in scan_runs (the previous lane's cell, a ballot of the heads); a run's violation is the
//                                        ballot of the violating lanes under the run's lane mask; the head lane issues the atomic.
//                                        The run that reaches the chunk's last lane is not flushed but CARRIED (cell, flag) into the
//                                        next chunk, where it goes on if lane 0's cell is the same.
//                The per-point counters and the two 64-bit totals are summed per workgroup in LDS (32 bits are enough there: at most
//                256 x 65536 samples): one global atomic per workgroup and counter, the wide ones as 64-bit integer atomics.
//   scan_clear_cells_kernel  one lane per roi cell: hits >= min_hits clears both layers, the hits go back to 0, cells_hit /
//                cells_cleared from ballots, the bounding box from a wavefront reduction; the last workgroup (scan_fuse_kernel's
//                ticket) takes the totals out with atomic exchanges that leave the rest values and writes fpe_scan_clear_info.
// No float atomics.
#pragma once

namespace {

// A point that casts a ray.  cls: 0 no point (a lane behind the last), 1 dropped, 2 long, 3 empty, 4 walked: samples k0 .. k1 - 1.
struct ClearRay {
    int32_t cls;
    int32_t k0, k1, K;
    double dx, dy, dz;
};

// The ray of a point that is cast, from the point where it has x, y, z (sensor frame): the fuse's tests 1-4, then the sample range.
__device__ __forceinline__ ClearRay clear_ray_of(const ScanClearArgs& a, float x, float y, float z) {
    ClearRay r{1, 0, 0, 0, 0.0, 0.0, 0.0};
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) return r;
    const double xs = x, ys = y, zs = z;
    const double r2 = (xs * xs + ys * ys) + zs * zs;
    if (!(a.minR2 <= r2 && r2 <= a.maxR2)) return r;
    const double xm = ((a.T[0] * xs + a.T[1] * ys) + a.T[2] * zs) + a.T[3];
    const double ym = ((a.T[4] * xs + a.T[5] * ys) + a.T[6] * zs) + a.T[7];
    const double zm = ((a.T[8] * xs + a.T[9] * ys) + a.T[10] * zs) + a.T[11];
    if (!(a.minZ <= zm && zm <= a.maxZ)) return r;
    r.dx = xm - a.T[3];
    r.dy = ym - a.T[7];
    r.dz = zm - a.T[11];
    const double Kd = ceil(fmax(fabs(r.dx), fabs(r.dy)) / a.step);
    r.cls = 2;
    if (!(Kd <= a.maxSamples)) return r;  // (a NaN of an overflowed transform counts as long too: it has no integer form)
    r.K = static_cast<int32_t>(Kd);
    r.k0 = a.startSamples;
    r.k1 = r.K - a.endSamples;
    r.cls = r.k0 < r.k1 ? 4 : 3;
    return r;
}

// The point source of the ray kernels (their template parameter): the x, y, z of point ordinal i.  This one reads the call's points;
// the image forms' source is fpe_scan_image.hpp's.
struct ClearPointSource {
    static __device__ __forceinline__ void xyz(const ScanClearArgs& a, int i, float& x, float& y, float& z) {
        const float* s = a.points + static_cast<size_t>(i) * static_cast<size_t>(a.stride);
        x = s[0];
        y = s[1];
        z = s[2];
    }
};

// Cast point c (ordinal c * ray_stride) as a ray.
template <class Source>
__device__ __forceinline__ ClearRay clear_ray(const ScanClearArgs& a, int c) {
    if (c >= a.nCast) return ClearRay{0, 0, 0, 0, 0.0, 0.0, 0.0};
    float x, y, z;
    Source::xyz(a, c * a.rayStride, x, y, z);  // (below n <= FPE_SCAN_MAX_POINTS)
    return clear_ray_of(a, x, y, z);
}

// Sample k of a walked ray: its local cell in the roi (kScanNoCell: not inside) and whether it violates that cell.
struct ClearSample {
    uint32_t cell;
    bool viol;
};

__device__ __forceinline__ ClearSample clear_sample(const ScanClearArgs& a, const ClearRay& r, int k) {
    ClearSample s{kScanNoCell, false};
    const double t = static_cast<double>(k) / static_cast<double>(r.K);
    const double x = a.T[3] + t * r.dx;
    const double y = a.T[7] + t * r.dy;
    const double z = a.T[11] + t * r.dz;
    if (!(within_axis(x, a.g.orgX, a.g.posX, a.g.lenX) && within_axis(y, a.g.orgY, a.g.posY, a.g.lenY))) return s;
    const int ci = index_of_fast(x, a.g.orgX, a.g.posX, a.g.res, a.g.rinv) - a.row0;  // (index_of's value: fpe_gridmath.hpp)
    const int cj = index_of_fast(y, a.g.orgY, a.g.posY, a.g.res, a.g.rinv) - a.col0;
    if (ci < 0 || ci >= a.nr || cj < 0 || cj >= a.nc) return s;
    s.cell = static_cast<uint32_t>(ci * a.nc + cj);
    const float h = __uint_as_float(a.elev[static_cast<size_t>(a.row0 + ci) * static_cast<size_t>(a.g.cols) + static_cast<size_t>(a.col0 + cj)]);
    s.viol = h == h && (z + a.margin) < static_cast<double>(h);
    return s;
}

__device__ __forceinline__ int32_t clear_wave_sum(int32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

// The workgroup's counters: sCnt[0..3] dropped, rays, long, empty; [4] samples inside, [5] (ray, cell) pairs.  Every lane calls;
// `counts` says whether the lane speaks for a point.  One LDS atomic per wavefront and counter, then one global atomic per workgroup.
__device__ __forceinline__ void clear_block_counts(const ScanClearArgs& a, int32_t* sCnt, bool counts, int32_t cls, int32_t nIn, int32_t nPairs) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int32_t dropped = __popcll(__ballot(counts && cls == 1));
    const int32_t rays = __popcll(__ballot(counts && cls >= 2));
    const int32_t longs = __popcll(__ballot(counts && cls == 2));
    const int32_t empties = __popcll(__ballot(counts && cls == 3));
    nIn = clear_wave_sum(nIn);
    nPairs = clear_wave_sum(nPairs);
    if (lane == 0) {
        if (dropped) atomicAdd(sCnt + 0, dropped);
        if (rays) atomicAdd(sCnt + 1, rays);
        if (longs) atomicAdd(sCnt + 2, longs);
        if (empties) atomicAdd(sCnt + 3, empties);
        if (nIn) atomicAdd(sCnt + 4, nIn);
        if (nPairs) atomicAdd(sCnt + 5, nPairs);
    }
    __syncthreads();
    const int w = static_cast<int>(threadIdx.x);
    if (w < 4) {
        if (sCnt[w]) atomicAdd(a.acc + kClearAccDropped + w, sCnt[w]);
    } else if (w < 6) {
        if (sCnt[w]) atomicAdd(reinterpret_cast<unsigned long long*>(a.acc + kClearAccWide) + (w - 4), static_cast<unsigned long long>(sCnt[w]));
    }
}

template <class Source>
__global__ __launch_bounds__(kScanBlock) void scan_clear_rays_lane_kernel(ScanClearArgs a) {
    __shared__ int32_t sCnt[6];
    if (threadIdx.x < 6) sCnt[threadIdx.x] = 0;
    __syncthreads();
    const ClearRay r = clear_ray<Source>(a, static_cast<int>(blockIdx.x) * kScanBlock + static_cast<int>(threadIdx.x));
    int32_t nIn = 0, nPairs = 0;
    if (r.cls == 4) {
        uint32_t cur = kScanNoCell;
        bool flag = false;  // (set only while cur is a cell)
        for (int k = r.k0; k < r.k1; ++k) {
            const ClearSample s = clear_sample(a, r, k);
            if (s.cell != cur) {
                if (flag) {
                    atomicAdd(&a.cells[cur].count, 1u);
                    ++nPairs;
                }
                cur = s.cell;
                flag = false;
            }
            if (s.cell != kScanNoCell) {
                ++nIn;
                flag |= s.viol;
            }
        }
        if (flag) {
            atomicAdd(&a.cells[cur].count, 1u);
            ++nPairs;
        }
    }
    clear_block_counts(a, sCnt, true, r.cls, nIn, nPairs);
}

template <int G, class Source>
__global__ __launch_bounds__(kScanBlock) void scan_clear_rays_group_kernel(ScanClearArgs a) {
    static_assert(G == 16 || G == 32 || G == 64, "a group is a power-of-two part of a wavefront");
    __shared__ int32_t sCnt[6];
    if (threadIdx.x < 6) sCnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int gl = lane & (G - 1);  // the lane within its group
    const int first = lane - gl;    // the group's first lane, and the one behind its last
    const int end = first + G;
    const unsigned long long below = (1ull << lane) - 1ull;  // the lanes below this one
    const unsigned long long group = (G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull) << first;
    const ClearRay r = clear_ray<Source>(a, static_cast<int>(blockIdx.x) * (kScanBlock / G) + static_cast<int>(threadIdx.x) / G);
    const int k1 = r.cls == 4 ? r.k1 : 0;
    uint32_t carryCell = kScanNoCell;  // the run that reached the last chunk's end (the same in every lane of the group)
    bool carryFlag = false;            // (set only while carryCell is a cell)
    int32_t nIn = 0, nPairs = 0;
    // (the trip count is the wavefront's: a group whose ray has ended goes along with no sample, which ends its carried run)
    for (int base = r.cls == 4 ? r.k0 : 0; __ballot(base < k1) != 0ull; base += G) {
        const int k = base + gl;
        ClearSample s{kScanNoCell, false};
        if (k < k1) s = clear_sample(a, r, k);
        if (s.cell != kScanNoCell) ++nIn;
        // runs of equal cells along the group's lanes (scan_runs' heads, with a head at every group's first lane)
        const uint32_t prev = __shfl_up(s.cell, 1);
        const bool head = gl == 0 || prev != s.cell;
        const unsigned long long heads = __ballot(head);
        const unsigned long long viol = __ballot(s.viol);
        // this lane's run, were it a head: from here to the next head (the next group's first lane is one) or the wavefront's end
        const unsigned long long above = heads & ~((below << 1) | 1ull);
        const int next = above ? __builtin_ctzll(above) : 64;
        const unsigned long long run = (next == 64 ? ~0ull : (1ull << next) - 1ull) & ~below;
        bool any = (viol & run) != 0ull;
        if (head) {
            if (gl == 0) {
                if (s.cell == carryCell) {
                    any |= carryFlag;  // the carried run goes on
                } else if (carryFlag) {
                    atomicAdd(&a.cells[carryCell].count, 1u);
                    ++nPairs;
                }
            }
            if (next != end && any) {  // (a run that reaches the group's end is carried, not flushed; `any` only of a cell's run)
                atomicAdd(&a.cells[s.cell].count, 1u);
                ++nPairs;
            }
        }
        // the carry of the next chunk: the group's last run
        const int lastHead = 63 - __builtin_clzll(heads & group);
        const uint32_t lastCell = __shfl(s.cell, end - 1);
        bool lastFlag = (viol & group & ~((1ull << lastHead) - 1ull)) != 0ull;
        if (lastHead == first && lastCell == carryCell) lastFlag |= carryFlag;
        carryCell = lastCell;
        carryFlag = lastFlag;
    }
    if (gl == 0 && carryFlag) {
        atomicAdd(&a.cells[carryCell].count, 1u);
        ++nPairs;
    }
    clear_block_counts(a, sCnt, gl == 0, r.cls, nIn, nPairs);
}

__global__ __launch_bounds__(kScanBlock) void scan_clear_cells_kernel(ScanClearArgs a) {
    __shared__ int32_t sLast;
    __shared__ int32_t sInfo[16];
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int idx = static_cast<int>(blockIdx.x) * kScanBlock + static_cast<int>(threadIdx.x);
    bool hit = false, gone = false;
    int i = 0, j = 0;
    if (idx < a.nr * a.nc) {
        const uint32_t hits = a.cells[idx].count;
        if (hits != 0u) {
            hit = true;
            if (hits >= static_cast<uint32_t>(a.minHits)) {
                gone = true;
                const int r = idx / a.nc;
                i = a.row0 + r;
                j = a.col0 + (idx - r * a.nc);
                const size_t k = static_cast<size_t>(i) * static_cast<size_t>(a.g.cols) + static_cast<size_t>(j);
                a.elev[k] = kScanCleared;
                a.var[k] = kScanCleared;
            }
            a.cells[idx].count = 0u;
        }
    }
    scan_count(hit, a.acc + kClearAccDropped + 4, lane);
    scan_count(gone, a.acc + kClearAccDropped + 5, lane);
    if (__ballot(gone) != 0ull) {  // (wave-uniform) the bounding box of the wavefront's cleared cells
        int rmin = gone ? i : INT32_MAX, cmin = gone ? j : INT32_MAX, rmax = gone ? i : -1, cmax = gone ? j : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            rmin = min(rmin, __shfl_xor(rmin, d));
            cmin = min(cmin, __shfl_xor(cmin, d));
            rmax = max(rmax, __shfl_xor(rmax, d));
            cmax = max(cmax, __shfl_xor(cmax, d));
        }
        if (lane == 0) {
            atomicMin(a.acc + 12, rmin);
            atomicMin(a.acc + 13, cmin);
            atomicMax(a.acc + 14, rmax);
            atomicMax(a.acc + 15, cmax);
        }
    }
    // scan_fuse_kernel's ticket: the last workgroup takes every total out with an exchange that leaves the rest value behind
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) sLast = atomicAdd(reinterpret_cast<uint32_t*>(a.acc + kScanTicket), 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!sLast) return;
    __threadfence();
    const int w = static_cast<int>(threadIdx.x);  // the info's word
    if (w < 16) {
        const int src = w < 2 ? -1 : w < 8 ? kClearAccDropped + (w - 2) : w < 12 ? 12 + (w - 8) : kClearAccWide + (w - 12);
        int32_t v = src >= 0 ? atomicExch(a.acc + src, scan_acc_rest(src)) : 0;
        if (w == 0) v = a.n;
        if (w == 1) v = a.n - a.nCast;  // strided out: known without looking
        sInfo[w] = v;
    }
    if (w == 16) atomicExch(a.acc + kScanTicket, 0);
    __syncthreads();
    if (w < 16 && a.info) {
        int32_t v = sInfo[w];
        if (w >= 8 && w < 12 && sInfo[7] == 0) v = w < 10 ? 0 : -1;  // no cleared cell: {0, 0, -1, -1}
        a.info[w] = v;
    }
}

// The ray pass of either point source.
template <class Source>
hipError_t clear_rays_launch(const ScanClearArgs& a, int form, int group, hipStream_t stream) {
    if (a.nCast <= 0) return hipSuccess;
    const size_t n = static_cast<size_t>(a.nCast);
    if (form == 1) {
        hipLaunchKernelGGL(scan_clear_rays_lane_kernel<Source>, dim3(scan_blocks(n)), dim3(kScanBlock), 0, stream, a);
    } else if (group == 16) {
        hipLaunchKernelGGL((scan_clear_rays_group_kernel<16, Source>), dim3(scan_blocks(n * 16)), dim3(kScanBlock), 0, stream, a);
    } else if (group == 32) {
        hipLaunchKernelGGL((scan_clear_rays_group_kernel<32, Source>), dim3(scan_blocks(n * 32)), dim3(kScanBlock), 0, stream, a);
    } else {
        hipLaunchKernelGGL((scan_clear_rays_group_kernel<64, Source>), dim3(scan_blocks(n * 64)), dim3(kScanBlock), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_scan_clear_rays(const ScanClearArgs& a, int form, int group, hipStream_t stream) {
    return clear_rays_launch<ClearPointSource>(a, form, group, stream);
}

// (runs for n == 0 too: it writes the caller's info)
hipError_t launch_scan_clear_cells(const ScanClearArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(scan_clear_cells_kernel, dim3(scan_blocks(static_cast<size_t>(a.nr) * static_cast<size_t>(a.nc))), dim3(kScanBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_scan_clear(const ScanClearArgs& a, int form, int group, hipStream_t stream) {
    hipError_t e = launch_scan_clear_rays(a, form, group, stream);
    if (e == hipSuccess) e = launch_scan_clear_cells(a, stream);
    return e;
}
