// laserscan_kernels.h -- geometry::LaserScanBuffer: scans -> points, points / depth pixels -> scans, the range and the
// shadow filter (laserscanbuffer.cu, laserscanbuffer_factory.cu, pointcloud_factory.cu CreateFromLaserScanBuffer).
// The contract is in include/mi_icp.h ("laserscan"); tests/laserscan_exact.py restates it in numpy.
//
// THE REDUCTION.  A bin of a virtual scan ends as the minimum range of the points that fall into it.  Ranges are >= 0,
// so their bit patterns order as unsigned integers, and the quiet NaN a bin starts as (0x7fc00000) lies above +inf's
// (0x7f800000): one unsigned atomic minimum per point over NaN-initialised bins is the whole reduction, whatever the
// order of arrival.  (The reference reads, compares and exchanges, so the smaller range can lose.)
//  LDS path    bins <= kLsLdsBins: every workgroup keeps the whole table in LDS (72 KiB: two workgroups share a CU's
//              160 KiB), takes a contiguous share of the points with ds atomic minima, and flushes the bins it touched
//              (those no longer NaN) with one global atomic minimum each.
//  global path atomics straight to memory.
#pragma once
#include "depth_kernels.h"
#include "device_utils.h"

namespace mi {

constexpr int kLsLdsBins = 18432;       // 72 KiB of bins per workgroup
constexpr int kLsMaxBins = 1 << 26;     // the largest steps x divisions an entry point takes
constexpr int kLsThreads = 1024;
constexpr int kLsPerThread = 16;        // points a thread of the LDS path takes at least (when there are that many)
constexpr uint32_t kLsNaN = 0x7fc00000u;

struct LsBins {
    float min_h, h_inc;  // heights (from_depth: min_y and its increment)
    float min_r, max_r, min_a, max_a, a_inc;
    int divisions, steps;
};

// the bin of a point of the scan frame and its range's bits; false: the point is dropped
__device__ __forceinline__ bool ls_bin(const LsBins& a, float x, float y, float z, int& bin, uint32_t& bits) {
    if (!(fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY)) return false;
    const float range = sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
    if (range < a.min_r || range > a.max_r) return false;
    const float angle = atan2f(y, x);
    if (angle < a.min_a || angle > a.max_a) return false;
    if (z < a.min_h) return false;
    const float fj = (z - a.min_h) / a.h_inc;
    const float fi = (angle - a.min_a) / a.a_inc;
    if (!(fj < 2.0e9f) || !(fi < 2.0e9f)) return false;  // (NaN too: the casts below are defined)
    const int j = (int)fj, i = (int)fi;
    if (j < 0 || i < 0 || j >= a.divisions || i >= a.steps) return false;
    bin = j * a.steps + i;
    bits = __float_as_uint(range);
    return true;
}

struct LsPointSource {
    const float* pts;
    __device__ __forceinline__ bool get(int64_t idx, float& x, float& y, float& z) const {
        x = pts[idx * 3];
        y = pts[idx * 3 + 1];
        z = pts[idx * 3 + 2];
        return true;
    }
};

// a depth pixel in the scan frame: the camera point (x, y, z) turned by the exact quarter turn about X, (x, -z, y)
struct LsDepthSource {
    DepthArgs d;
    __device__ __forceinline__ bool get(int64_t idx, float& x, float& y, float& z) const {
        int row, col;
        strided_pixel(d, idx, row, col);
        const float dz = depth_value(d, (int64_t)row * d.width + col);
        if (dz <= 0.0f) return false;
        x = ((float)col - d.cx) * dz / d.fx;
        z = ((float)row - d.cy) * dz / d.fy;
        y = -dz;
        return true;
    }
};

static __global__ __launch_bounds__(256) void ls_fill_u32(uint32_t* __restrict__ p, int64_t n, uint32_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

template <class Source>
__global__ __launch_bounds__(kLsThreads) void ls_bin_lds(Source src, int64_t n, int64_t per_block, LsBins a, uint32_t* __restrict__ out) {
    __shared__ uint32_t tab[kLsLdsBins];
    const int bins = a.divisions * a.steps;
    for (int b = threadIdx.x; b < bins; b += kLsThreads) tab[b] = kLsNaN;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * per_block;
    const int64_t hi = lo + per_block < n ? lo + per_block : n;
    for (int64_t idx = lo + threadIdx.x; idx < hi; idx += kLsThreads) {
        float x, y, z;
        int bin;
        uint32_t bits;
        if (src.get(idx, x, y, z) && ls_bin(a, x, y, z, bin, bits)) atomicMin(&tab[bin], bits);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kLsThreads) {
        const uint32_t v = tab[b];
        if (v != kLsNaN) atomicMin(&out[b], v);
    }
}

template <class Source>
__global__ __launch_bounds__(256) void ls_bin_global(Source src, int64_t n, LsBins a, uint32_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    float x, y, z;
    int bin;
    uint32_t bits;
    if (src.get(idx, x, y, z) && ls_bin(a, x, y, z, bin, bits)) atomicMin(&out[bin], bits);
}

// ---- scans -> points -----------------------------------------------------------------------------------------------
struct LsScans {
    const float* ranges;       // [num_max_scans][num_steps]
    const float* intensities;  // the same shape, or null
    const float* cs;           // [num_steps][2]: cos, sin of the step's angle (host table)
    const float* origins;      // [num_scans][12]: per LIVE scan O(r,0), O(r,1), O(r,3) for r = 0..2, then three spare words
    int steps, max_scans, first, scans;
    float min_r, max_r;
};

// the point of reading e = k * steps + i of the live scans; false: not kept, or not finite
__device__ __forceinline__ bool ls_point(const LsScans& a, int64_t e, float p[3], float& v) {
    const int k = (int)(e / a.steps), i = (int)(e % a.steps);
    const int64_t at = (int64_t)((a.first + k) % a.max_scans) * a.steps + i;
    const float r = a.ranges[at];
    if (!(!isnan(r) && !(r < a.min_r) && !(a.max_r < r))) return false;
    const float x = __fmul_rn(r, a.cs[i * 2]), y = __fmul_rn(r, a.cs[i * 2 + 1]);
    const float* O = a.origins + (int64_t)k * 12;
#pragma unroll
    for (int q = 0; q < 3; ++q) p[q] = __fadd_rn(__fadd_rn(__fmul_rn(O[q * 3], x), __fmul_rn(O[q * 3 + 1], y)), O[q * 3 + 2]);
    v = a.intensities ? a.intensities[at] : 0.0f;
    return finite3(p);
}

static __global__ __launch_bounds__(256) void ls_point_flags(LsScans a, int64_t count, uint32_t* __restrict__ flags) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    float p[3], v;
    flags[e] = ls_point(a, e, p, v) ? 1u : 0u;
}

static __global__ __launch_bounds__(256) void ls_point_emit(LsScans a, int64_t count, const uint32_t* __restrict__ pos,
                                                     float* __restrict__ out_xyz, float* __restrict__ out_rgb) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    float p[3], v;
    if (!ls_point(a, e, p, v)) return;
    const int64_t o = (int64_t)pos[e];
    out_xyz[o * 3] = p[0];
    out_xyz[o * 3 + 1] = p[1];
    out_xyz[o * 3 + 2] = p[2];
    if (out_rgb) out_rgb[o * 3] = out_rgb[o * 3 + 1] = out_rgb[o * 3 + 2] = v;
}

// ---- filters -------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void ls_range_filter(const float* __restrict__ r, int64_t count, float min_r, float max_r,
                                                       float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float v = r[e];
    out[e] = (v < min_r || v > max_r) ? __uint_as_float(kLsNaN) : v;
}

// out is a copy of r on entry; every write is the same NaN, so the writers' order is free.  cs: [2 * window + 1][2]
static __global__ __launch_bounds__(256) void ls_shadow_filter(const float* __restrict__ r, int64_t count, int steps, int window,
                                                        int neighbors, int remove_start, float min_tan, float max_tan,
                                                        const float* __restrict__ cs, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const int i = (int)(e % steps);
    const float* row = r + (e - i);
    float* orow = out + (e - i);
    const float ri = row[i];
    bool shadow = false;
    for (int y = -window; y <= window && !shadow; ++y) {
        const int j = i + y;
        if (j < 0 || j >= steps || j == i) continue;
        const float rj = row[j];
        const float py = __fmul_rn(rj, cs[(y + window) * 2 + 1]);
        const float px = __fsub_rn(ri, __fmul_rn(rj, cs[(y + window) * 2]));
        const float t = fabsf(py) / px;
        shadow = (t > 0.0f) ? (t < min_tan) : (t > max_tan);
    }
    if (!shadow) return;  // (one shadow or several: the same bins get the same NaN)
    const int lo = i - neighbors > 0 ? i - neighbors : 0, hi = i + neighbors < steps - 1 ? i + neighbors : steps - 1;
    for (int index = lo; index <= hi; ++index)
        if (ri < row[index]) orow[index] = __uint_as_float(kLsNaN);
    if (remove_start) orow[i] = __uint_as_float(kLsNaN);
}

static __global__ __launch_bounds__(256) void ls_scale(float* __restrict__ r, int64_t count, float s) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) r[e] = __fmul_rn(r[e], s);
}

}  // namespace mi
