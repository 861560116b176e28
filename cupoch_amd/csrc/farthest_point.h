// farthest_point.h -- PointCloud::FarthestPointDownSample (geometry/pointcloud.cu:122-139, 301-338).
//
// The reference: per sample a thrust::transform_reduce over the whole cloud (the distance update and an argmax whose
// ties fall to the reduction's order) and a device-to-host copy of the chosen index.  Here a sample is ONE launch,
// fps_step, and the launches of a call are enqueued back to back -- the chosen index and its coordinates stay in device
// memory, the host waits once, at the end of the call:
//   fps_init    sel[0] = 0, its coordinates into cur[0], the ticket cleared.
//   fps_step t  every thread streams points and dist once (12 B read of the point, 4 B read of dist and 4 B written where
//               it changed: at most 20 B per point; launch 0 takes +inf for dist instead of reading it), dist = min(dist, d2(i, sel[t])),
//               and keeps its best as the packed key (dist bits << 32) | ~i: a non-negative fp32 orders as its bits,
//               so one unsigned 64-bit max is "largest dist, lowest index".  Keys are reduced over the wave on the DPP
//               network, over the block through LDS; the block's key goes to partial[block] write-through, and the
//               LAST block to take the ticket (reduce.h's hand-off) folds the partials the same way and writes
//               sel[t + 1] and its coordinates into cur[(t + 1) & 1] for the next launch.
// A max of integers has no order to fix: the same input gives the same sel on every run, grid and context.
// The contract is stated in include/mi_icp.h (mi_icp_farthest_point_downsample).
#pragma once
#include "device_utils.h"

namespace mi {

constexpr int kFpsThreads = 256;
constexpr int kFpsMaxBlocks = 1024;  // partial[] entries; the finishing block reads 4 per thread
constexpr int kFpsUnroll = 4;        // points a thread has in flight

// device state of one call: [0, kFpsMaxBlocks) the blocks' keys, then the ticket and the chosen point's coordinates
struct FpsState {
    unsigned long long partial[kFpsMaxBlocks];
    float cur[2][4];
    uint32_t ticket;
    uint32_t pad[7];
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_hop_u64(unsigned long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo;
}
__device__ __forceinline__ unsigned long long max_u64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// the wave's largest key, in lane kWaveSumLane (wave_sum's network; a lane without a source receives 0, below every key)
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    v = max_u64(v, dpp_hop_u64<0x111, 0xf>(v));  // row_shr:1
    v = max_u64(v, dpp_hop_u64<0x112, 0xf>(v));  // row_shr:2
    v = max_u64(v, dpp_hop_u64<0x114, 0xf>(v));  // row_shr:4
    v = max_u64(v, dpp_hop_u64<0x118, 0xf>(v));  // row_shr:8
    v = max_u64(v, dpp_hop_u64<0x142, 0xa>(v));  // row_bcast:15
    v = max_u64(v, dpp_hop_u64<0x143, 0xc>(v));  // row_bcast:31
    return v;
}

// the block's largest key, returned to thread 0 (red: kFpsThreads / 64 words of LDS; a barrier inside)
__device__ __forceinline__ unsigned long long fps_block_max(unsigned long long key, unsigned long long* red) {
    key = wave_max_u64(key);
    if (lane_id() == kWaveSumLane) red[threadIdx.x >> 6] = key;
    __syncthreads();
    unsigned long long m = 0ull;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kFpsThreads / 64; ++w) m = max_u64(m, red[w]);
    }
    return m;
}

__device__ __forceinline__ unsigned long long fps_key(float dist, int64_t i) {
    return ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned long long)(~(uint32_t)i);
}

static __global__ __launch_bounds__(64) void fps_init(const float* __restrict__ pts, FpsState* __restrict__ st,
                                                     int64_t* __restrict__ sel) {
    const int t = (int)threadIdx.x;
    if (t < 3) st->cur[0][t] = pts[t];
    if (t == 3) st->ticket = 0u;
    if (t == 4) sel[0] = 0;
}

// the identity selection of num_samples == n
static __global__ __launch_bounds__(256) void fps_iota(int64_t* __restrict__ sel, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) sel[i] = i;
}

// Sample t + 1 from sample t.  FIRST: dist is +inf everywhere and is not read.  Grid: at most kFpsMaxBlocks blocks.
template <bool FIRST>
__global__ __launch_bounds__(kFpsThreads) void fps_step(const float* __restrict__ pts, float* __restrict__ dist, int64_t n,
                                                        int64_t t, FpsState* __restrict__ st, int64_t* __restrict__ sel) {
    __shared__ unsigned long long red[kFpsThreads / 64];
    __shared__ uint32_t s_last;
    const float* cur = st->cur[t & 1];
    const float cx = cur[0], cy = cur[1], cz = cur[2];
    // Every key of a point is at least ~i > 0, so 0 is "no point".  dist >= 0 and never NaN: d2 is a sum of squares, and
    // fminf returns its other argument when d2 is NaN (a non-finite coordinate), which leaves +inf standing.
    unsigned long long best = 0ull;
    const int64_t stride = (int64_t)gridDim.x * kFpsThreads;
    for (int64_t i0 = (int64_t)blockIdx.x * kFpsThreads + threadIdx.x; i0 < n; i0 += stride * kFpsUnroll) {
        float x[kFpsUnroll], y[kFpsUnroll], z[kFpsUnroll], d[kFpsUnroll];
#pragma unroll
        for (int u = 0; u < kFpsUnroll; ++u) {
            const int64_t i = i0 + u * stride;
            const bool in = i < n;
            const float* p = pts + (in ? i : i0) * 3;
            x[u] = p[0];
            y[u] = p[1];
            z[u] = p[2];
            d[u] = FIRST ? INFINITY : dist[in ? i : i0];
        }
#pragma unroll
        for (int u = 0; u < kFpsUnroll; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n) {
                const float v = fminf(d[u], sq3(x[u] - cx, y[u] - cy, z[u] - cz));
                if (FIRST || v != d[u]) dist[i] = v;  // (most points keep their distance once a few samples are out)
                best = max_u64(best, fps_key(v, i));
            }
        }
    }
    const unsigned long long mine = fps_block_max(best, red);
    if (threadIdx.x == 0) {
        // reduce.h's hand-off: the key stored write-through, drained, then the ticket; the last block acquires
        __hip_atomic_store(&st->partial[blockIdx.x], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t k = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = k == gridDim.x - 1u;
        if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_last = last ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    unsigned long long all = 0ull;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += kFpsThreads) all = max_u64(all, st->partial[b]);
    __syncthreads();  // (red is written again)
    all = fps_block_max(all, red);
    if (threadIdx.x == 0) {
        int64_t j = (int64_t)(~(uint32_t)all);
        if (j >= n) j = 0;  // (cannot happen with n >= 1: every point offers a key; kept as the bound of the loads below)
        sel[t + 1] = j;
        float* nxt = st->cur[(t + 1) & 1];
        nxt[0] = pts[j * 3];
        nxt[1] = pts[j * 3 + 1];
        nxt[2] = pts[j * 3 + 2];
        __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace mi
