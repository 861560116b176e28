// segment_plane.h -- PointCloud::SegmentPlane (geometry/segmentation.cu:187-268): RANSAC plane fit, all hypotheses at once.
//
// The reference runs, per iteration, a tabulate of n random keys, a sort of all n indices (to read the first three), a
// copy of three points to the host, a copy_if over all n points and a reduce.  The hypotheses do not depend on each
// other, so here (the contract is in include/mi_icp.h):
//   seg_hypotheses   one thread per iteration: the triple (a pure function of seed, t, n), its plane, a valid flag
//   seg_score        THE hot kernel: every point against every hypothesis in one pass over the points -> count[H]
//   seg_select       one wave: the largest count of a valid hypothesis, and the list of hypotheses that reach it
//   seg_tie_partial  only when several tie: their fp64 error sums, per block (fixed order)
//   seg_pick         one wave: the winner (count, then error sum, then iteration); its plane into the state
//   seg_flags        the winner's inlier flags, from the same distance expression as seg_score
//   exclusive_scan_u32 + seg_list: the inlier indices, ascending, int64
//   seg_centroid_partial / seg_centroid_final, seg_moments_partial / seg_refit_final: GetPlaneFromPoints in fp64
// The number of launches does not depend on the iteration count, and nothing comes back to the host before the end.
#pragma once
#include "device_utils.h"
#include "fgr_rules.h"

namespace mi {

constexpr int kSegPoints = 8;                       // points a lane of seg_score keeps in registers
constexpr int kSegChunk = 256 * kSegPoints;         // points of one block's pass over the hypotheses
constexpr int kSegTile = 2048;                      // hypotheses whose counters a block keeps in LDS at a time
constexpr int kSegMaxBlocks = 1024;                 // seg_score's persistent grid: 4 blocks per CU
constexpr int kSegTieBlocks = 64;                   // blocks (per tied hypothesis) of seg_tie_partial
constexpr int kSegRefitBlocks = 512;                // blocks of the refit's two reductions at most
constexpr int64_t kSegMaxIterations = 65536;        // (the tie pass keeps kSegTieBlocks doubles per hypothesis)

struct SegState {
    float ransac[4];      // the winning hypothesis' plane, (0,0,0,0) when there is none
    float refit[4];       // GetPlaneFromPoints of its inliers
    int32_t best;         // its iteration, -1: none
    uint32_t best_count;  // its inliers as seg_score counted them, 0: none
    uint32_t max_count;   // seg_select: the largest count of a valid hypothesis
    uint32_t tied;        // ... and how many reach it (their iterations: tied_list, ascending)
};

// ---- the sampler (include/mi_icp.h): u(j) = output j of splitmix64 seeded with `seed` -------------------------------
__host__ __device__ inline uint64_t seg_u(uint64_t seed, uint64_t j) { return fgr::stream_u(seed, j); }  // (fgr_rules.h)

__device__ __forceinline__ uint64_t seg_below(uint64_t u, uint64_t m) { return __umul64hi(u, m); }  // floor(u * m / 2^64)

// three distinct indices of [0, n), n >= 3: the head of a uniform random permutation
__device__ __forceinline__ void seg_triple(uint64_t seed, uint64_t t, uint64_t n, uint64_t* i0, uint64_t* i1, uint64_t* i2) {
    const uint64_t a = seg_below(seg_u(seed, 3 * t), n);
    uint64_t b = seg_below(seg_u(seed, 3 * t + 1), n - 1);
    if (b >= a) ++b;
    uint64_t c = seg_below(seg_u(seed, 3 * t + 2), n - 2);
    const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
    if (c >= lo) ++c;
    if (c >= hi) ++c;
    *i0 = a;
    *i1 = b;
    *i2 = c;
}

// ---- the one distance expression: a x + b y + c z + d as three fused multiply-adds, d first ------------------------
__device__ __forceinline__ float seg_signed(float a, float b, float c, float d, float x, float y, float z) {
    return __builtin_fmaf(c, z, __builtin_fmaf(b, y, __builtin_fmaf(a, x, d)));
}
__device__ __forceinline__ bool seg_inlier(float a, float b, float c, float d, float x, float y, float z, float thr) {
    return __builtin_fabsf(seg_signed(a, b, c, d, x, y, z)) < thr;
}

// ComputeTrianglePlane (segmentation.cu:60-74) in fp32, nothing contracted.  valid iff 0 < norm < inf.
static __global__ __launch_bounds__(256) void seg_hypotheses(const float* __restrict__ xyz, int64_t n, uint64_t seed, int H,
                                                            float4* __restrict__ plane, uint32_t* __restrict__ valid) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= H) return;
    uint64_t i[3];
    seg_triple(seed, (uint64_t)t, (uint64_t)n, &i[0], &i[1], &i[2]);
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) p[k][d] = xyz[i[k] * 3 + d];
    const float e0x = p[1][0] - p[0][0], e0y = p[1][1] - p[0][1], e0z = p[1][2] - p[0][2];
    const float e1x = p[2][0] - p[0][0], e1y = p[2][1] - p[0][1], e1z = p[2][2] - p[0][2];
    float a = e0y * e1z - e0z * e1y;
    float b = e0z * e1x - e0x * e1z;
    float c = e0x * e1y - e0y * e1x;
    const float norm = sqrtf((a * a + b * b) + c * c);
    const bool ok = norm > 0.0f && norm < INFINITY;
    float4 pl = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ok) {
        a = a / norm;
        b = b / norm;
        c = c / norm;
        pl = make_float4(a, b, c, -((a * p[0][0] + b * p[0][1]) + c * p[0][2]));
    }
    plane[t] = pl;
    valid[t] = ok ? 1u : 0u;
}

// count[h] += #{i : |plane_h . (p_i, 1)| < thr}, for every hypothesis, in one pass over the points.
// A block takes chunks of kSegChunk points, kSegPoints per lane in registers.  The hypotheses are the outer loop: the
// plane is wave-uniform and comes through scalar loads (the next one asked for before this one is used), the compare's
// lane mask is popcounted on the scalar side, and the wave's count of hypothesis h0 + j is kept by lane j of one VGPR
// (a compare and a select), so 64 hypotheses cost ONE LDS add per wave.  The block's counters stay in LDS for a whole
// tile of kSegTile hypotheses and are flushed once, with integer atomics: no order can change the result.
// More than kSegTile hypotheses: the block walks its chunks once per tile.
struct SegPlane {
    float a, b, c, d;
};
__device__ __forceinline__ SegPlane seg_plane_at(cfloat_p plane, int h) {
    return SegPlane{plane[h * 4], plane[h * 4 + 1], plane[h * 4 + 2], plane[h * 4 + 3]};
}

// one chunk against the hypotheses [h_tile, h_tile + ht).  kFull: all kSegChunk points exist; else the points past the
// end load the last point and their lanes are masked out of every ballot.
template <bool kFull>
__device__ __forceinline__ void seg_score_chunk(const float* __restrict__ xyz, int64_t n, int64_t first, cfloat_p plane,
                                                int h_tile, int ht, float thr, uint32_t* cnt) {
    const int lane = lane_id();
    float x[kSegPoints], y[kSegPoints], z[kSegPoints];
    bool in[kSegPoints];
#pragma unroll
    for (int p = 0; p < kSegPoints; ++p) {
        const int64_t i = first + p * 256 + threadIdx.x;
        in[p] = kFull || i < n;
        const int64_t ic = in[p] ? i : n - 1;  // (every load unconditional: all of a chunk's are in flight together)
        x[p] = xyz[ic * 3];
        y[p] = xyz[ic * 3 + 1];
        z[p] = xyz[ic * 3 + 2];
    }
    for (int h0 = 0; h0 < ht; h0 += 64) {
        const int hn = min(64, ht - h0);
        uint32_t acc = 0u;  // lane j: this wave's count of hypothesis h_tile + h0 + j
        SegPlane next = seg_plane_at(plane, h_tile + h0);
        for (int j = 0; j < hn; ++j) {
            const SegPlane pl = next;
            next = seg_plane_at(plane, h_tile + h0 + min(j + 1, hn - 1));
            uint32_t s = 0u;
#pragma unroll
            for (int p = 0; p < kSegPoints; ++p) {
                uint64_t m = __ballot(seg_inlier(pl.a, pl.b, pl.c, pl.d, x[p], y[p], z[p], thr));
                if (!kFull) m &= __ballot(in[p]);
                s += (uint32_t)__builtin_popcountll(m);
            }
            acc = lane == j ? s : acc;
        }
        if (lane < hn && acc) atomicAdd(&cnt[h0 + lane], acc);
    }
}

static __global__ __launch_bounds__(256) void seg_score(const float* __restrict__ xyz, int64_t n, const float4* __restrict__ plane_g,
                                                       int H, float thr, uint32_t* __restrict__ count) {
    __shared__ uint32_t cnt[kSegTile];
    const cfloat_p plane = (cfloat_p)(uintptr_t)plane_g;
    const int64_t nchunks = (n + kSegChunk - 1) / kSegChunk;
    for (int h_tile = 0; h_tile < H; h_tile += kSegTile) {
        const int ht = min(kSegTile, H - h_tile);
        for (int k = (int)threadIdx.x; k < ht; k += 256) cnt[k] = 0u;
        __syncthreads();
        for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
            const int64_t first = chunk * kSegChunk;
            if (first + kSegChunk <= n) seg_score_chunk<true>(xyz, n, first, plane, h_tile, ht, thr, cnt);
            else seg_score_chunk<false>(xyz, n, first, plane, h_tile, ht, thr, cnt);
        }
        __syncthreads();
        for (int k = (int)threadIdx.x; k < ht; k += 256)
            if (cnt[k]) atomicAdd(&count[h_tile + k], cnt[k]);
        __syncthreads();
    }
}

// One wave: the largest count >= 1 of a valid hypothesis, and the iterations that reach it, ascending.  None (no valid
// hypothesis, or none with an inlier -- the reference's `fitness > 0` never holds then): tied = 0.
static __global__ __launch_bounds__(64) void seg_select(const uint32_t* __restrict__ count, const uint32_t* __restrict__ valid,
                                                       int H, SegState* __restrict__ st, int32_t* __restrict__ tied_list) {
    const int lane = lane_id();
    uint32_t mx = 0u;
    for (int h = lane; h < H; h += 64)
        if (valid[h]) mx = max(mx, count[h]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    uint32_t T = 0u;
    if (mx > 0u) {
        for (int h0 = 0; h0 < H; h0 += 64) {
            const int h = h0 + lane;
            const bool hit = h < H && valid[h] && count[h] == mx;
            const uint64_t m = __ballot(hit);
            if (hit) tied_list[T + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = h;
            T += (uint32_t)__builtin_popcountll(m);
        }
    }
    if (lane == 0) {
        st->max_count = mx;
        st->tied = T;
    }
}

// Hypotheses tied at the largest count: the fp64 sum of the inliers' fp32 distances.  Block (bx, by) adds, for the tied
// hypotheses by, by + gridDim.y, ..., the points bx * 256 + tid, + 256 * kSegTieBlocks, ...: per thread in that order,
// wave_sum over the lanes, the four waves in order.  seg_pick adds the blocks in order.  A single winner: nothing to do.
static __global__ __launch_bounds__(256) void seg_tie_partial(const float* __restrict__ xyz, int64_t n,
                                                             const float4* __restrict__ plane, float thr,
                                                             const SegState* __restrict__ st,
                                                             const int32_t* __restrict__ tied_list,
                                                             double* __restrict__ partial /*[tied][kSegTieBlocks]*/) {
    __shared__ double red[4];
    const uint32_t T = st->tied;
    if (T < 2u) return;
    const int lane = lane_id(), wid = (int)(threadIdx.x >> 6);
    for (uint32_t t = blockIdx.y; t < T; t += gridDim.y) {
        const float4 pl = plane[tied_list[t]];
        double s = 0.0;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kSegTieBlocks * 256) {
            const float dist = __builtin_fabsf(seg_signed(pl.x, pl.y, pl.z, pl.w, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]));
            if (dist < thr) s += (double)dist;
        }
        s = wave_sum(s);
        if (lane == kWaveSumLane) red[wid] = s;
        __syncthreads();
        if (threadIdx.x == 0) partial[(size_t)t * kSegTieBlocks + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
    }
}

// One wave: among the tied hypotheses the smallest error sum, among equal sums the lowest iteration.
static __global__ __launch_bounds__(64) void seg_pick(const float4* __restrict__ plane, const int32_t* __restrict__ tied_list,
                                                     const double* __restrict__ partial, SegState* __restrict__ st) {
    const int lane = lane_id();
    const uint32_t T = st->tied;
    uint32_t best_t = 0u;
    if (T >= 2u) {
        double bs = INFINITY;
        uint32_t bt = 0xffffffffu;
        for (uint32_t t = lane; t < T; t += 64) {  // (ascending per lane: `<` keeps the lowest iteration)
            double s = 0.0;
            for (int b = 0; b < kSegTieBlocks; ++b) s += partial[(size_t)t * kSegTieBlocks + b];
            if (s < bs) {
                bs = s;
                bt = t;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o, 64);
            const uint32_t ot = (uint32_t)__shfl_xor((int)bt, o, 64);
            if (os < bs || (os == bs && ot < bt)) {
                bs = os;
                bt = ot;
            }
        }
        best_t = bt;
    }
    if (lane != 0) return;
    if (T == 0u) {
        st->ransac[0] = st->ransac[1] = st->ransac[2] = st->ransac[3] = 0.0f;
        st->best = -1;
        st->best_count = 0u;
        return;
    }
    const int32_t h = tied_list[best_t];
    const float4 pl = plane[h];
    st->ransac[0] = pl.x;
    st->ransac[1] = pl.y;
    st->ransac[2] = pl.z;
    st->ransac[3] = pl.w;
    st->best = h;
    st->best_count = st->max_count;
}

// the winner's inliers (segmentation.cu:245-260); with no winner the plane is zero and every finite point's distance is 0
static __global__ __launch_bounds__(256) void seg_flags(const float* __restrict__ xyz, int64_t n, const SegState* __restrict__ st,
                                                       float thr, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = seg_inlier(st->ransac[0], st->ransac[1], st->ransac[2], st->ransac[3], xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], thr)
                       ? 1u
                       : 0u;
}

static __global__ __launch_bounds__(256) void seg_list(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                                      int64_t n, int64_t* __restrict__ out_idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flags[i]) out_idx[pos[i]] = i;
}

// ---- GetPlaneFromPoints (segmentation.cu:135-185) in fp64 -----------------------------------------------------------
// a block's sums of D values per flagged point, the grid striding over the points: per thread in order, wave_sum, the
// four waves in order -> partial[block][8]
template <int D, class F>
__device__ __forceinline__ void seg_block_sums(const uint32_t* __restrict__ flags, int64_t n, double* __restrict__ partial, F value) {
    __shared__ double red[4][D];
    double s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        if (flags[i]) value(i, s);
    const int lane = lane_id(), wid = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double v = wave_sum(s[d]);
        if (lane == kWaveSumLane) red[wid][d] = v;
    }
    __syncthreads();
    if (threadIdx.x < D) {
        const int d = (int)threadIdx.x;
        partial[blockIdx.x * 8 + d] = ((red[0][d] + red[1][d]) + red[2][d]) + red[3][d];
    }
}

// one wave adds the blocks' partials: lane l the blocks l, l + 64, ... in order, then wave_sum (as outlier_stats_final)
template <int D>
__device__ __forceinline__ void seg_final_sums(const double* __restrict__ partial, int nblocks, double* out) {
    double s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = 0.0;
    for (int b = lane_id(); b < nblocks; b += 64)
#pragma unroll
        for (int d = 0; d < D; ++d) s[d] += partial[b * 8 + d];
#pragma unroll
    for (int d = 0; d < D; ++d) out[d] = __shfl(wave_sum(s[d]), kWaveSumLane, 64);
}

static __global__ __launch_bounds__(256) void seg_centroid_partial(const float* __restrict__ xyz, const uint32_t* __restrict__ flags,
                                                                  int64_t n, double* __restrict__ partial) {
    seg_block_sums<4>(flags, n, partial, [&](int64_t i, double* s) {
        s[0] += (double)xyz[i * 3];
        s[1] += (double)xyz[i * 3 + 1];
        s[2] += (double)xyz[i * 3 + 2];
        s[3] += 1.0;
    });
}

// centroid[0..2] = the sums / the count, centroid[3] = the count
static __global__ __launch_bounds__(64) void seg_centroid_final(const double* __restrict__ partial, int nblocks,
                                                               double* __restrict__ centroid) {
    double s[4];
    seg_final_sums<4>(partial, nblocks, s);
    if (lane_id() != 0) return;
    const double m = s[3];
    for (int d = 0; d < 3; ++d) centroid[d] = m > 0.0 ? s[d] / m : 0.0;
    centroid[3] = m;
}

// the six centred second moments xx, xy, xz, yy, yz, zz
static __global__ __launch_bounds__(256) void seg_moments_partial(const float* __restrict__ xyz, const uint32_t* __restrict__ flags,
                                                                 int64_t n, const double* __restrict__ centroid,
                                                                 double* __restrict__ partial) {
    const double cx = centroid[0], cy = centroid[1], cz = centroid[2];
    seg_block_sums<6>(flags, n, partial, [&](int64_t i, double* s) {
        const double rx = (double)xyz[i * 3] - cx, ry = (double)xyz[i * 3 + 1] - cy, rz = (double)xyz[i * 3 + 2] - cz;
        s[0] += rx * rx;
        s[1] += rx * ry;
        s[2] += rx * rz;
        s[3] += ry * ry;
        s[4] += ry * rz;
        s[5] += rz * rz;
    });
}

// segmentation.cu:158-184: the largest of the three 2x2 determinants picks the branch; normalised; d = -abc . centroid.
// All of it in fp64, rounded to fp32 once.  No inliers, or a zero norm: the zero plane.
static __global__ __launch_bounds__(64) void seg_refit_final(const double* __restrict__ partial, int nblocks,
                                                            const double* __restrict__ centroid, SegState* __restrict__ st) {
    double m[6];
    seg_final_sums<6>(partial, nblocks, m);
    if (lane_id() != 0) return;
    const double det_x = m[3] * m[5] - m[4] * m[4];
    const double det_y = m[0] * m[5] - m[2] * m[2];
    const double det_z = m[0] * m[3] - m[1] * m[1];
    double a, b, c;
    if (det_x > det_y && det_x > det_z) {
        a = det_x;
        b = m[2] * m[4] - m[1] * m[5];
        c = m[1] * m[4] - m[2] * m[3];
    } else if (det_y > det_z) {
        a = m[2] * m[4] - m[1] * m[5];
        b = det_y;
        c = m[1] * m[2] - m[4] * m[0];
    } else {
        a = m[1] * m[4] - m[2] * m[3];
        b = m[1] * m[2] - m[4] * m[0];
        c = det_z;
    }
    const double norm = sqrt((a * a + b * b) + c * c);
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (centroid[3] > 0.0 && norm > 0.0 && norm < (double)INFINITY) {
        a /= norm;
        b /= norm;
        c /= norm;
        out[0] = (float)a;
        out[1] = (float)b;
        out[2] = (float)c;
        out[3] = (float)(-((a * centroid[0] + b * centroid[1]) + c * centroid[2]));
    }
    for (int k = 0; k < 4; ++k) st->refit[k] = out[k];
}

}  // namespace mi
