// select.h -- the tails of the outlier filters and the index selections (geometry/down_sample.cu:40-62,110-129,
// 317-438): PointCloud::RemoveStatisticalOutliers' statistics and threshold, the keep flags of both filters, and one
// gather that serves them and SelectByIndex.
//
// The reference: per-point k-NN / radius lists written out (KDTreeFlann::SearchKNN / SearchRadius), a transform_reduce
// per statistic, copy_if over an enumeration, then SelectByIndex.  Here knn_normals_kernel<2 | 3> leaves one number
// per point (the mean squared distance, the count), and the rest is:
//   statistical:  outlier_stats_partial (per-block fp64 sums) -> outlier_stats_final (one wave: the threshold, on the
//                 device) -> outlier_flags_stat
//   radius:       outlier_flags_radius
//   both:         exclusive_scan_u32 of the flags -> select_gather (points, normals, colours and the original index of
//                 every kept point at its scanned position, ascending in original index)
//   SelectByIndex: select_list (a gather in the order given) or, with invert, select_mark (flags start at 1, the named
//                 indices clear theirs) and the same scan + select_gather.
//   SelectByMask:  select_mask_flags (a byte per point -> the flags) and the same scan + select_gather.
//   PassThroughFilter / Crop / RemoveNoneFinitePoints (geometry/pointcloud.cu:40-54, 108-120, 340-348):
//                 pass_through_flags / crop_flags / finite_flags and the same scan + select_gather.
// Every sum has a fixed order (per block, then the blocks in a fixed order): the same input gives the same threshold on
// every run and every context.  Indices outside [0, n) are reported in a status word that comes back with the count.
#pragma once
#include "device_utils.h"

namespace mi {

constexpr int kOutlierBlocks = 512;  // blocks of outlier_stats_partial at most (the partials: [blocks][4] doubles)

// Σ avg, Σ avg², #{avg > 0} of this block's points.  avg >= 0 everywhere, so the zeros add nothing to either sum and
// the reference's "over the points with avg > 0" (down_sample.cu:405-412) needs only the count.
static __global__ __launch_bounds__(256) void outlier_stats_partial(const float* __restrict__ avg, int64_t n,
                                                                   double* __restrict__ partial /*[blocks][4]*/) {
    __shared__ double red[4][3];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double a = (double)avg[i];
        s[0] += a;
        s[1] += a * a;
        s[2] += a > 0.0 ? 1.0 : 0.0;
    }
    const int lane = lane_id(), wid = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double v = wave_sum(s[d]);
        if (lane == kWaveSumLane) red[wid][d] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int d = (int)threadIdx.x;
        partial[blockIdx.x * 4 + d] = ((red[0][d] + red[1][d]) + red[2][d]) + red[3][d];
    }
}

// One wave: thr = mean + std_ratio * std (down_sample.cu:395-418), with
//   valid = n (every point finds itself), mean = Σ avg / valid,
//   sq = Σ_{avg>0} (avg - mean)² = Σ avg² - 2 mean Σ avg + #{avg>0} mean²  (the expanded form of the reference's sum,
//        from the same sums; clamped at 0 against cancellation),
//   std = sqrt(sq / (valid - 1)).
// Lane l adds the partials of blocks l, l + 64, ... in order, wave_sum the lanes in its fixed order (one thread walking
// all 512 partials was 72 us of dependent loads at 10M points).  Fewer than 2 points: thr = -inf, nothing is kept (the
// reference's 0/0 keeps nothing either).
static __global__ __launch_bounds__(64) void outlier_stats_final(const double* __restrict__ partial, int nblocks,
                                                                int64_t n, double std_ratio, double* __restrict__ thr) {
    const int lane = lane_id();
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = lane; b < nblocks; b += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] += partial[b * 4 + d];
    }
    const double s1 = wave_sum(s[0]), s2 = wave_sum(s[1]), pos = wave_sum(s[2]);
    if (lane != kWaveSumLane) return;
    if (n < 2) {
        *thr = -INFINITY;
        return;
    }
    const double valid = (double)n;
    const double mean = s1 / valid;
    const double sq = fmax(s2 - 2.0 * mean * s1 + pos * mean * mean, 0.0);
    const double sd = sqrt(sq / (valid - 1.0));
    *thr = mean + std_ratio * sd;
}

// keep iff avg > 0 && avg < thr (down_sample.cu:420-426), compared in fp64
static __global__ __launch_bounds__(256) void outlier_flags_stat(const float* __restrict__ avg, int64_t n,
                                                                const double* __restrict__ thr,
                                                                uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = avg[i];
    flags[i] = (a > 0.0f && (double)a < *thr) ? 1u : 0u;
}

// keep iff the radius search found `need` = nb_points + 1 points, the point itself included (down_sample.cu:336-343)
static __global__ __launch_bounds__(256) void outlier_flags_radius(const int32_t* __restrict__ count, int64_t n, int need,
                                                                  uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = count[i] >= need ? 1u : 0u;
}

// (a 12-byte record moves the same whether it holds floats or ints: T is float for a cloud, int32_t for a VoxelGrid's keys)
template <typename T>
__device__ __forceinline__ void copy3(const T* __restrict__ src, int64_t i, T* __restrict__ dst, int64_t p) {
    dst[p * 3] = src[i * 3];
    dst[p * 3 + 1] = src[i * 3 + 1];
    dst[p * 3 + 2] = src[i * 3 + 2];
}

// Every flagged point i to position pos[i] (exclusive scan of the flags): its point, normal and colour (those given),
// and i itself into out_idx when that is given.
template <typename T>
static __global__ __launch_bounds__(256) void select_gather(const uint32_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ pos, int64_t n,
                                                           const T* __restrict__ xyz, const float* __restrict__ nrm,
                                                           const float* __restrict__ col, T* __restrict__ oxyz,
                                                           float* __restrict__ onrm, float* __restrict__ ocol,
                                                           int64_t* __restrict__ out_idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const int64_t p = pos[i];
    copy3(xyz, i, oxyz, p);
    if (nrm) copy3(nrm, i, onrm, p);
    if (col) copy3(col, i, ocol, p);
    if (out_idx) out_idx[p] = i;
}

// SelectByIndex(indices): entry j of the output is point indices[j].  An index outside [0, n) sets *status and writes
// nothing.
template <typename T>
static __global__ __launch_bounds__(256) void select_list(const int64_t* __restrict__ idx, int64_t n_idx, int64_t n,
                                                         const T* __restrict__ xyz, const float* __restrict__ nrm,
                                                         const float* __restrict__ col, T* __restrict__ oxyz,
                                                         float* __restrict__ onrm, float* __restrict__ ocol,
                                                         uint32_t* __restrict__ status) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_idx) return;
    const int64_t i = idx[j];
    if (i < 0 || i >= n) {
        atomicOr(status, 1u);
        return;
    }
    copy3(xyz, i, oxyz, j);
    if (nrm) copy3(nrm, i, onrm, j);
    if (col) copy3(col, i, ocol, j);
}

// SelectByIndex(indices, invert = true): the named points' flags (all 1 before) are cleared -- a repeated index clears
// the same flag again.  An index outside [0, n) sets *status.
static __global__ __launch_bounds__(256) void select_mark(const int64_t* __restrict__ idx, int64_t n_idx, int64_t n,
                                                         uint32_t* __restrict__ flags, uint32_t* __restrict__ status) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_idx) return;
    const int64_t i = idx[j];
    if (i < 0 || i >= n) {
        atomicOr(status, 1u);
        return;
    }
    flags[i] = 0u;
}

// SelectByMask's flags: entry i is kept iff (mask[i] != 0) != invert
static __global__ __launch_bounds__(256) void select_mask_flags(const uint8_t* __restrict__ mask, int64_t n, int invert,
                                                               uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = ((mask[i] != 0) != (invert != 0)) ? 1u : 0u;
}

// PassThroughFilter's flags: kept iff !(v < lo || hi < v), v = p[axis] -- a NaN coordinate is kept, as the reference's
// comparison keeps it
static __global__ __launch_bounds__(256) void pass_through_flags(const float* __restrict__ xyz, int64_t n, int axis, float lo,
                                                                float hi, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = xyz[i * 3 + axis];
    flags[i] = (v < lo || hi < v) ? 0u : 1u;
}

struct CropBox {
    float lo[3], hi[3];
};

// Crop(AxisAlignedBoundingBox)'s flags: kept iff on all three axes !(p < lo || p > hi) -- bounds inclusive, NaN kept
static __global__ __launch_bounds__(256) void crop_flags(const float* __restrict__ xyz, int64_t n, CropBox b,
                                                        uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    const bool out = (x < b.lo[0] || x > b.hi[0]) || (y < b.lo[1] || y > b.hi[1]) || (z < b.lo[2] || z > b.hi[2]);
    flags[i] = out ? 0u : 1u;
}

// RemoveNoneFinitePoints' flags: dropped iff (remove_nan and a coordinate is NaN) or (remove_inf and one is +-inf)
static __global__ __launch_bounds__(256) void finite_flags(const float* __restrict__ xyz, int64_t n, int remove_nan,
                                                          int remove_inf, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    const bool has_nan = x != x || y != y || z != z;
    const bool has_inf = fabsf(x) == INFINITY || fabsf(y) == INFINITY || fabsf(z) == INFINITY;
    flags[i] = ((remove_nan && has_nan) || (remove_inf && has_inf)) ? 0u : 1u;
}

}  // namespace mi
