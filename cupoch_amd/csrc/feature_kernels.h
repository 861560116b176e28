// feature_kernels.h -- registration::Feature matching and FastGlobalRegistration (registration/fast_global_registration.cu,
// knn/bruteforce_nn.inl); the contract is in include/mi_icp.h, the host/device rules in fgr_rules.h.
//
// The reference materialises the ref x query distance matrix twice (40 GB at 100k x 100k) and takes its row minima.
// Here:
//   feature_match_kernel  THE hot kernel: one pass over the pair space gives the row minima AND the column minima,
//                         as 64-bit atomic minima on (float bits of D) << 32 | index; the matrix is never written
//   fm_decode             keys -> index / distance lists
//   fgr_recip_flags / fgr_recip_list    the reciprocal pairs, ascending in the source index (scan in between)
//   fgr_trial_flags / fgr_trial_emit    the tuple test of every trial, then only the first ceil(max / 3) passing ones
//                                       are written (scan in between)
//   fgr_sum_partial / fgr_mean_final / fgr_center_max / fgr_scales / fgr_divide    NormalizePointCloud
//   fgr_optimize_kernel   ONE workgroup runs all iterations: fp64 sums, the 6x6 solve by a wave (wave_solver.h), the
//                         fp32 point update, the par schedule -- no host round trip between iterations
//   fgr_finish            GetInvTransformationOriginalScale
#pragma once
#include "device_utils.h"
#include "fgr_rules.h"
#include "wave_solver.h"

namespace mi {

constexpr int kFmTile = 128;              // queries and refs of a block's tile
constexpr int kFmLane = 8;                // a lane's register tile: kFmLane x kFmLane pairs (16 x 16 lanes a block)
constexpr int kFmK = 16;                  // dimensions staged through LDS per trip
constexpr int kFmStride = kFmTile + 4;    // floats of an LDS row (rows stay 16-byte aligned, the staging writes spread over the banks)
constexpr int kFmMaxBlocks = 1 << 20;     // the grid at most; a block strides over the tiles
constexpr unsigned long long kFmNone = ~0ull;  // no finite-or-infinite distance seen: above every key
constexpr int kFgrSumBlocks = 256;        // blocks of the mean's partial sums at most
constexpr int kFgrMinCorres = 10;         // fast_global_registration.cu:321

__device__ __forceinline__ unsigned long long fm_key(float d, uint32_t idx) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)idx;
}

// row / column r = 0 .. 7 of a lane's register tile within the block's tile: two runs of four, 64 apart, so that the
// sixteen lanes of a row of lanes read 256 contiguous bytes with every ds_read_b128
__device__ __forceinline__ int fm_slot(int t, int r) { return (r < 4 ? 0 : 64) + t * 4 + (r & 3); }

// D(i, j) = sum over k in order of fma(e, e, acc), e = Q[i][k] - R[j][k] (one rounding), for the tile's 128 x 128
// pairs: lane (tx, ty) keeps 8 x 8 accumulators, both operand tiles are staged k-major through LDS, 16 dimensions a
// trip, the next trip's global loads in flight while this one is computed.  Dimensions past dim and rows past the
// end are staged as 0: fma(0, 0, acc) = acc exactly, and such rows are masked out of the minima.  Two waves per SIMD:
// the 64 accumulators, the staged operands and the epilogue's keys need ~230 VGPRs; bounded to 128 the kernel spills.
static __global__ __launch_bounds__(256, 2) void feature_match_kernel(const float* __restrict__ Q, int64_t nq, const float* __restrict__ R,
                                                                  int64_t nr, int dim, int64_t tiles_r, int64_t tiles,
                                                                  unsigned long long* __restrict__ qkey,
                                                                  unsigned long long* __restrict__ rkey) {
    __shared__ __attribute__((aligned(16))) float qs[kFmK][kFmStride];
    __shared__ __attribute__((aligned(16))) float rs[kFmK][kFmStride];
    __shared__ unsigned long long rmin[kFmTile];
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t q0 = (tile / tiles_r) * kFmTile, r0 = (tile % tiles_r) * kFmTile;
        if (tid < kFmTile) rmin[tid] = kFmNone;
        float acc[kFmLane][kFmLane];
#pragma unroll
        for (int i = 0; i < kFmLane; ++i)
#pragma unroll
            for (int j = 0; j < kFmLane; ++j) acc[i][j] = 0.0f;
        float gq[8], gr[8];  // staging: element e of this thread is (row (e * 256 + tid) / 16, dimension (e * 256 + tid) % 16)
        auto fetch = [&](int k0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int idx = e * 256 + tid, row = idx >> 4, k = k0 + (idx & 15);
                const int64_t qi = q0 + row, ri = r0 + row;
                gq[e] = (qi < nq && k < dim) ? Q[qi * dim + k] : 0.0f;
                gr[e] = (ri < nr && k < dim) ? R[ri * dim + k] : 0.0f;
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < dim; k0 += kFmK) {
            __syncthreads();  // the last trip's reads are over
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int idx = e * 256 + tid, row = idx >> 4, kk = idx & 15;
                qs[kk][row] = gq[e];
                rs[kk][row] = gr[e];
            }
            __syncthreads();
            if (k0 + kFmK < dim) fetch(k0 + kFmK);
#pragma unroll 4
            for (int kk = 0; kk < kFmK; ++kk) {
                float a[kFmLane], b[kFmLane];
                *(float4*)&a[0] = *(const float4*)&qs[kk][ty * 4];
                *(float4*)&a[4] = *(const float4*)&qs[kk][64 + ty * 4];
                *(float4*)&b[0] = *(const float4*)&rs[kk][tx * 4];
                *(float4*)&b[4] = *(const float4*)&rs[kk][64 + tx * 4];
#pragma unroll
                for (int i = 0; i < kFmLane; ++i)
#pragma unroll
                    for (int j = 0; j < kFmLane; ++j) {
                        const float e = a[i] - b[j];
                        acc[i][j] = __builtin_fmaf(e, e, acc[i][j]);
                    }
            }
        }
        // row minima: a row's 128 refs lie in the sixteen lanes tx = 0 .. 15 of one ty (consecutive lanes)
#pragma unroll
        for (int i = 0; i < kFmLane; ++i) {
            unsigned long long key = kFmNone;
#pragma unroll
            for (int j = 0; j < kFmLane; ++j) {
                const int64_t rj = r0 + fm_slot(tx, j);
                const float d = acc[i][j];
                if (rj < nr && d == d) key = min(key, fm_key(d, (uint32_t)rj));  // (a NaN never wins)
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) key = min(key, (unsigned long long)__shfl_xor(key, o, 64));
            const int64_t qi = q0 + fm_slot(ty, i);
            if (tx == 0 && qi < nq && key != kFmNone) atomicMin(&qkey[qi], key);
        }
        // column minima: a column's 128 queries lie in the sixteen ty, four of them in this wave (lane bits 4, 5)
#pragma unroll
        for (int j = 0; j < kFmLane; ++j) {
            unsigned long long key = kFmNone;
#pragma unroll
            for (int i = 0; i < kFmLane; ++i) {
                const int64_t qi = q0 + fm_slot(ty, i);
                const float d = acc[i][j];
                if (qi < nq && d == d) key = min(key, fm_key(d, (uint32_t)qi));
            }
            key = min(key, (unsigned long long)__shfl_xor(key, 16, 64));
            key = min(key, (unsigned long long)__shfl_xor(key, 32, 64));
            if ((tid & 48) == 0 && key != kFmNone) atomicMin(&rmin[fm_slot(tx, j)], key);
        }
        __syncthreads();
        if (tid < kFmTile) {
            const int64_t rj = r0 + tid;
            const unsigned long long key = rmin[tid];
            if (rj < nr && key != kFmNone) atomicMin(&rkey[rj], key);
        }
    }
}

// idx / d (either may be null): the neighbour and its distance; no neighbour (every distance a NaN): -1 and a NaN
static __global__ __launch_bounds__(256) void fm_decode(const unsigned long long* __restrict__ key, int64_t n, int32_t* __restrict__ idx,
                                                       float* __restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    if (idx) idx[i] = k == kFmNone ? -1 : (int32_t)(uint32_t)k;
    if (d) d[i] = k == kFmNone ? __uint_as_float(0x7fc00000u) : __uint_as_float((uint32_t)(k >> 32));
}

// flags[i] = 1 iff source row i has a neighbour j in [0, nt) and (reciprocal != 0) j's neighbour is i
static __global__ __launch_bounds__(256) void fgr_recip_flags(const int32_t* __restrict__ s_idx, int64_t ns, const int32_t* __restrict__ t_idx,
                                                             int64_t nt, int reciprocal, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    const int32_t j = s_idx[i];
    const bool has = j >= 0 && (int64_t)j < nt;
    flags[i] = (has && (!reciprocal || (int64_t)t_idx[j] == i)) ? 1u : 0u;
}

static __global__ __launch_bounds__(256) void fgr_recip_list(const int32_t* __restrict__ s_idx, int64_t ns, const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ pos, int32_t* __restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns || !flags[i]) return;
    pairs[2 * (size_t)pos[i]] = (int32_t)i;
    pairs[2 * (size_t)pos[i] + 1] = s_idx[i];
}

// the three pairs of trial t and whether it passes the tuple test (fgr_rules.h); a pair whose index lies outside
// its cloud fails the trial
__device__ __forceinline__ bool fgr_trial(const int32_t* __restrict__ pairs, uint64_t ncorr, const float* __restrict__ src, int64_t ns,
                                          const float* __restrict__ tgt, int64_t nt, uint64_t seed, uint64_t t, float s2, int32_t* ij) {
    bool in = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const uint64_t a = fgr::trial_pair(seed, t, m, ncorr);
        ij[2 * m] = pairs[2 * a];
        ij[2 * m + 1] = pairs[2 * a + 1];
        in = in && ij[2 * m] >= 0 && ij[2 * m] < ns && ij[2 * m + 1] >= 0 && ij[2 * m + 1] < nt;
    }
    if (!in) return false;
    float p[3][3], q[3][3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            p[m][d] = src[(size_t)ij[2 * m] * 3 + d];
            q[m][d] = tgt[(size_t)ij[2 * m + 1] * 3 + d];
        }
    return fgr::tuple_ok(p[0], p[1], p[2], q[0], q[1], q[2], s2);
}

static __global__ __launch_bounds__(256) void fgr_trial_flags(const int32_t* __restrict__ pairs, int64_t ncorr, const float* __restrict__ src,
                                                             int64_t ns, const float* __restrict__ tgt, int64_t nt, uint64_t seed, float s2,
                                                             int64_t trials, uint32_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= trials) return;
    int32_t ij[6];
    flags[t] = fgr_trial(pairs, (uint64_t)ncorr, src, ns, tgt, nt, seed, (uint64_t)t, s2, ij) ? 1u : 0u;
}

// passing trial number pos[t] writes its correspondences 3 pos[t] .. 3 pos[t] + 2, those below max_corr; *n_out =
// min(3 * passing trials, max_corr)
static __global__ __launch_bounds__(256) void fgr_trial_emit(const int32_t* __restrict__ pairs, int64_t ncorr, uint64_t seed, int64_t trials,
                                                            const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                                            const uint32_t* __restrict__ total, int64_t max_corr, int32_t* __restrict__ corr,
                                                            uint32_t* __restrict__ n_out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *n_out = (uint32_t)fgr::cut_count((int64_t)*total, max_corr);
    if (t >= trials || !flags[t]) return;
    const int64_t first = 3 * (int64_t)pos[t];
    if (first >= max_corr) return;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (first + m >= max_corr) break;
        const uint64_t a = fgr::trial_pair(seed, (uint64_t)t, m, (uint64_t)ncorr);
        corr[2 * (first + m)] = pairs[2 * a];
        corr[2 * (first + m) + 1] = pairs[2 * a + 1];
    }
}

// ---- NormalizePointCloud (fast_global_registration.cu:197-265) ------------------------------------------------------
// fp64 sums of x, y, z: per thread in order (the grid striding over the points), wave_sum, the four waves in order
static __global__ __launch_bounds__(256) void fgr_sum_partial(const float* __restrict__ xyz, int64_t n, double* __restrict__ partial) {
    __shared__ double red[4][3];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] += (double)xyz[i * 3 + d];
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

// one wave: lane l adds the blocks l, l + 64, ... in order, then wave_sum; mean = (float)(sum / n)
static __global__ __launch_bounds__(64) void fgr_mean_final(const double* __restrict__ partial, int nblocks, int64_t n, float* __restrict__ mean3) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = lane_id(); b < nblocks; b += 64)
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] += partial[b * 4 + d];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double v = wave_sum(s[d]);
        if (lane_id() == kWaveSumLane) mean3[d] = (float)(v / (double)n);
    }
}

// out = p - mean; *max_bits = the bits of the largest squared norm (x*x + y*y) + z*z so far (a NaN takes no part)
static __global__ __launch_bounds__(256) void fgr_center_max(const float* __restrict__ xyz, int64_t n, const float* __restrict__ mean3,
                                                            float* __restrict__ out, uint32_t* __restrict__ max_bits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float n2 = 0.0f;
    if (i < n) {
        const float x = xyz[i * 3] - mean3[0], y = xyz[i * 3 + 1] - mean3[1], z = xyz[i * 3 + 2] - mean3[2];
        out[i * 3] = x;
        out[i * 3 + 1] = y;
        out[i * 3 + 2] = z;
        n2 = (x * x + y * y) + z * z;
        if (!(n2 == n2)) n2 = 0.0f;
    }
    uint32_t b = __float_as_uint(n2);  // (non-negative floats order as their bits)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, o, 64));
    if (lane_id() == 0 && b) atomicMax(max_bits, b);
}

// scales[0] = scale_global, scales[1] = the largest norm (scale_start of an absolute-scale call)
static __global__ void fgr_scales(const uint32_t* __restrict__ max_bits, int use_absolute_scale, float* __restrict__ scales) {
    const float scale = sqrtf(__uint_as_float(*max_bits));
    scales[0] = use_absolute_scale ? 1.0f : scale;
    scales[1] = scale;
}

static __global__ __launch_bounds__(256) void fgr_divide(float* __restrict__ xyz, int64_t n3, const float* __restrict__ scales) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n3) xyz[i] = xyz[i] / scales[0];
}

// ---- OptimizePairwiseRegistration (fast_global_registration.cu:267-372) --------------------------------------------
// One workgroup, every iteration.  Correspondence c = (i, j): p = src[i], q = this call's moving copy of tgt[j] (qwork,
// one slot per correspondence: thread tid owns the slots tid, tid + 256, ...).  Per iteration:
//   weight  r = p - q, w = (par / (((rx*rx + ry*ry) + rz*rz) + par))^2 in fp32, every operation rounded
//   sums    the 21 upper-triangle entries of JTJ and the 6 of JTr of the reference's three-row Jacobian, each term
//           formed and added in fp64 from the fp32 p, q, r, w: per thread in order, wave_sum, the four waves in order.
//           (fp32 roundings behind one term, against exact arithmetic on the same fp32 p, q, par: r 1; its square 2,
//           the three products' sum 2 + 1 + 2 = 5, + par 6, the division 7, squared 15; times r 16.  c = 16.)
//   solve   (-JTJ) x = JTr by wave 0 (wave_solve_update: JTJ x = -JTr, the same bits), delta = TransformVector6fToMatrix4f(x)
//   update  trans = delta * trans (mul4); q = ((d00 x + d01 y) + d02 z) + t0, ... in fp32, nothing fused
//   par     fgr::par_next
// A correspondence with an index outside its cloud takes no part.  count < 10 or no iteration: identity, zero sums.
static __global__ __launch_bounds__(256) void fgr_optimize_kernel(const float* __restrict__ src, int64_t ns, const float* __restrict__ tgt,
                                                                 int64_t nt, const int32_t* __restrict__ corr, int64_t count_host,
                                                                 const uint32_t* __restrict__ count_dev, float par_host,
                                                                 const float* __restrict__ par_dev, int iterations, int decrease_mu,
                                                                 float max_dist, float division_factor, float* __restrict__ qwork,
                                                                 float* __restrict__ T16, double* __restrict__ sums27,
                                                                 float* __restrict__ par_out) {
    __shared__ double red[4][27];
    __shared__ double sys[32];
    __shared__ float dl[16];
    const int tid = (int)threadIdx.x, lane = lane_id(), wid = tid >> 6;
    const int64_t count = count_dev ? (int64_t)*count_dev : count_host;
    float par = par_dev ? *par_dev : par_host;
    host::Mat4 trans = host::identity4();  // (wave 0's copy is the one written out)
    if (tid < 32) sys[tid] = 0.0;
    const bool run = count >= kFgrMinCorres && iterations > 0;
    if (run) {
        for (int64_t c = tid; c < count; c += 256) {
            const int32_t j = corr[2 * c + 1];
            const bool in = j >= 0 && j < nt;
#pragma unroll
            for (int d = 0; d < 3; ++d) qwork[c * 3 + d] = in ? tgt[(size_t)j * 3 + d] : 0.0f;
        }
        for (int itr = 0; itr < iterations; ++itr) {
            double s[27];
#pragma unroll
            for (int k = 0; k < 27; ++k) s[k] = 0.0;
            for (int64_t c = tid; c < count; c += 256) {
                const int32_t i = corr[2 * c], j = corr[2 * c + 1];
                if (i < 0 || i >= ns || j < 0 || j >= nt) continue;
                const float px = src[(size_t)i * 3], py = src[(size_t)i * 3 + 1], pz = src[(size_t)i * 3 + 2];
                const float qx = qwork[c * 3], qy = qwork[c * 3 + 1], qz = qwork[c * 3 + 2];
                const float rx = px - qx, ry = py - qy, rz = pz - qz;
                const float temp = par / (((rx * rx + ry * ry) + rz * rz) + par);
                const double W = (double)(temp * temp);
                const double X = qx, Y = qy, Z = qz, RX = rx, RY = ry, RZ = rz;
                s[0] += W * (Z * Z) + W * (Y * Y);  // (0,0)
                s[1] -= W * (Y * X);                // (0,1)
                s[2] -= W * (Z * X);                // (0,2)
                s[4] -= W * Z;                      // (0,4)
                s[5] += W * Y;                      // (0,5)
                s[6] += W * (Z * Z) + W * (X * X);  // (1,1)
                s[7] -= W * (Z * Y);                // (1,2)
                s[8] += W * Z;                      // (1,3)
                s[10] -= W * X;                     // (1,5)
                s[11] += W * (Y * Y) + W * (X * X); // (2,2)
                s[12] -= W * Y;                     // (2,3)
                s[13] += W * X;                     // (2,4)
                s[15] += W;                         // (3,3); (4,4) and (5,5) are copies
                s[21] += W * (Z * RY) - W * (Y * RZ);
                s[22] += W * (X * RZ) - W * (Z * RX);
                s[23] += W * (Y * RX) - W * (X * RY);
                s[24] -= W * RX;
                s[25] -= W * RY;
                s[26] -= W * RZ;
            }
            s[18] = s[15];
            s[20] = s[15];
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                const double v = wave_sum(s[k]);
                if (lane == kWaveSumLane) red[wid][k] = v;
            }
            __syncthreads();
            if (tid < 27) sys[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            __syncthreads();
            if (wid == 0) {
                const host::Mat4 delta = wave_solve_update(sys);
                trans = host::mul4(delta, trans);
                if (lane == 0)
                    for (int k = 0; k < 16; ++k) dl[k] = delta[k];
            }
            __syncthreads();
            float d[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) d[k] = dl[k];  // column-major: d[c * 4 + r]
            for (int64_t c = tid; c < count; c += 256) {
                const float x = qwork[c * 3], y = qwork[c * 3 + 1], z = qwork[c * 3 + 2];
                qwork[c * 3] = ((d[0] * x + d[4] * y) + d[8] * z) + d[12];
                qwork[c * 3 + 1] = ((d[1] * x + d[5] * y) + d[9] * z) + d[13];
                qwork[c * 3 + 2] = ((d[2] * x + d[6] * y) + d[10] * z) + d[14];
            }
            par = fgr::par_next(par, itr, decrease_mu != 0, max_dist, division_factor);
            // (sys and dl are rewritten only behind the next iteration's first barrier)
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < 16; ++k) T16[k] = trans[k];
        if (par_out) *par_out = par;
    }
    if (sums27 && tid < 27) sums27[tid] = sys[tid];
}

// GetInvTransformationOriginalScale (fast_global_registration.cu:376-389) in fp32, nothing fused: with R, t of trans,
// v = (-(R m1) + t * scale_global) + m0, out = [R^T, -(R^T v)]; rows of a product summed left to right
static __global__ void fgr_finish(const float* __restrict__ trans16, const float* __restrict__ mean_src, const float* __restrict__ mean_tgt,
                                  const float* __restrict__ scales, float* __restrict__ out16) {
    const float sg = scales[0];
    float v[3];
    for (int r = 0; r < 3; ++r) {
        const float rm = (trans16[0 * 4 + r] * mean_tgt[0] + trans16[1 * 4 + r] * mean_tgt[1]) + trans16[2 * 4 + r] * mean_tgt[2];
        v[r] = (-rm + trans16[12 + r] * sg) + mean_src[r];
    }
    for (int k = 0; k < 16; ++k) out16[k] = 0.0f;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out16[c * 4 + r] = trans16[r * 4 + c];  // R^T
        out16[12 + r] = -((trans16[r * 4 + 0] * v[0] + trans16[r * 4 + 1] * v[1]) + trans16[r * 4 + 2] * v[2]);
    }
    out16[15] = 1.0f;
}

}  // namespace mi
