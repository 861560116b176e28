// sgm_kernels.h -- imageproc::SemiGlobalMatching and PointCloud::CreateFromDisparity (the contract: include/mi_icp.h
// "stereo"; the numpy restatement: tests/sgm_exact.py).  Everything up to the disparity image is integer arithmetic.
//   sgm_census     per pixel the 31-bit centre-symmetric census word of a 9 x 7 window (both images in one launch)
//   sgm_paths<DPL> every path cost L_r of every direction in ONE launch: a wave walks one line of one direction, lane l
//                  holds the DPL = D / 64 disparities l * DPL .. l * DPL + DPL - 1 of the pixel before in registers.
//                  Horizontal lines are rows; a vertical or diagonal line starts at a column of the first (last) row and
//                  goes down (up) a row a step, a diagonal moving a column sideways and wrapping round the side border,
//                  where its path starts anew -- so the W waves of a direction touch W neighbouring pixels of one row at
//                  about the same time, and every store is the D contiguous bytes of one pixel.  A step's census loads
//                  are issued two steps ahead of their use.  The matching cost is
//                  formed here from the two census planes (one popcount); L(d - 1), L(d + 1) come from the neighbouring
//                  lanes by a wave shift on the DPP network, min_k L by a DPP reduction; nothing goes through LDS.
//   sgm_wta<DPL>   per pixel S = sum of the path bytes (never stored), the left map with the uniqueness test, and the
//                  right map's candidates: (S << 8 | d) goes by an LDS minimum to column x - d - min_disp of the block's
//                  row tile, the tile's minima by a global minimum to the frame's plane.  Minima of integers: any order
//                  gives the same words.
//   sgm_tail       3 x 3 median of both maps, left-right check, the 8-bit disparity
//   sgm_sums       S as uint16 [y][x][d] (tests: mi_icp_sgm_get_sums)
//   disparity_points  CreateFromDisparity
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mi {

constexpr int kSgmDropped = 0x3fff;  // stands in for a term of the recurrence that is dropped (d - 1 < 0, d + 1 >= D)
constexpr int kSgmTile = 64;         // pixels of a row that one block of sgm_wta takes
constexpr uint32_t kSgmNoCandidate = 0xffffffffu;
constexpr uint16_t kSgmInvalid = 0xffffu;

// direction r of the contract's list: (0,1), (0,-1), (1,0), (-1,0), (1,1), (1,-1), (-1,1), (-1,-1) as (dy, dx)
__host__ __device__ __forceinline__ int sgm_dir_dy(int r) { return r < 2 ? 0 : ((r == 2 || r == 4 || r == 5) ? 1 : -1); }
__host__ __device__ __forceinline__ int sgm_dir_dx(int r) { return r == 0 ? 1 : (r == 1 ? -1 : (r < 4 ? 0 : ((r & 1) ? -1 : 1))); }

static __global__ __launch_bounds__(256) void sgm_census(const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1, int W, int H,
                                                         uint32_t* __restrict__ dst0, uint32_t* __restrict__ dst1) {
    const uint8_t* __restrict__ src = blockIdx.z ? src1 : src0;
    uint32_t* __restrict__ dst = blockIdx.z ? dst1 : dst0;
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    uint32_t word = 0;
    if (y >= 3 && y < H - 3 && x >= 4 && x < W - 4) {
        const uint8_t* c = src + (size_t)y * W + x;
        int k = 0;
#pragma unroll
        for (int dy = -3; dy <= 0; ++dy) {
#pragma unroll
            for (int dx = -4; dx <= 4; ++dx) {
                if (dy == 0 && dx >= 0) break;
                word |= (uint32_t)(c[(ptrdiff_t)dy * W + dx] > c[-(ptrdiff_t)dy * W - dx]) << k;
                ++k;
            }
        }
    }
    dst[(size_t)y * W + x] = word;
}

// lanes without a source keep `old`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int sgm_dpp(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false);
}
// the wave's minimum, in every lane.  Lanes without a source take INT_MAX, the minimum's identity: the compiler folds each
// hop into one v_min_i32 with a DPP operand.
__device__ __forceinline__ int sgm_wave_min(int v) {
    constexpr int kTop = 0x7fffffff;
    v = min(v, sgm_dpp<0x111, 0xf>(kTop, v));  // row_shr:1
    v = min(v, sgm_dpp<0x112, 0xf>(kTop, v));  // row_shr:2
    v = min(v, sgm_dpp<0x114, 0xf>(kTop, v));  // row_shr:4
    v = min(v, sgm_dpp<0x118, 0xf>(kTop, v));  // row_shr:8
    v = min(v, sgm_dpp<0x142, 0xa>(kTop, v));  // row_bcast:15
    v = min(v, sgm_dpp<0x143, 0xc>(kTop, v));  // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

template <int DPL>
struct SgmPack;
template <>
struct SgmPack<1> { using type = uint8_t; };
template <>
struct SgmPack<2> { using type = uint16_t; };
template <>
struct SgmPack<4> { using type = uint32_t; };

// the census words lane `d0 ..` needs at pixel (y, x): the left one and the right ones at x - d - min_disp (0 left of the
// image; the load itself is clamped to column 0, so that no lane branches).  `vzero` is a zero the compiler cannot see
// through: it keeps the left word a vector load, which the loop can leave in flight, where a scalar load is waited for
// at once.
template <int DPL>
__device__ __forceinline__ void sgm_load_census(const uint32_t* __restrict__ cenL, const uint32_t* __restrict__ cenR, size_t row, int x,
                                                int shift, int vzero, uint32_t* cl, uint32_t* cr) {
    *cl = cenL[row + (size_t)(x + vzero)];
#pragma unroll
    for (int k = 0; k < DPL; ++k) {
        const int xr = x - shift - k;
        const uint32_t v = cenR[row + (size_t)max(xr, 0)];
        cr[k] = xr >= 0 ? v : 0u;
    }
}

// the pixel after (y, x) on a line of direction (dy, dx): a diagonal wraps round the side border
__device__ __forceinline__ void sgm_advance(int* x, int* y, int dx, int dy, int W) {
    int xn = *x + dx;
    if (xn >= W) xn = 0;
    if (xn < 0) xn = W - 1;
    *x = xn;
    *y += dy;
}

template <int DPL>
static __global__ __launch_bounds__(256) void sgm_paths(const uint32_t* __restrict__ cenL, const uint32_t* __restrict__ cenR, int W, int H,
                                                        int min_disp, int p1, int p2, uint8_t* __restrict__ vol, size_t vol_stride) {
    constexpr int D = 64 * DPL;
    using Pack = typename SgmPack<DPL>::type;
    const int lane = (int)(threadIdx.x & 63);
    const int line = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = (int)blockIdx.y;
    const int dy = sgm_dir_dy(r), dx = sgm_dir_dx(r);
    int x, y, steps;
    if (dy == 0) {
        if (line >= H) return;
        y = line;
        x = dx > 0 ? 0 : W - 1;
        steps = W;
    } else {
        if (line >= W) return;
        y = dy > 0 ? 0 : H - 1;
        x = line;
        steps = H;
    }
    Pack* __restrict__ out = reinterpret_cast<Pack*>(vol + (size_t)r * vol_stride) + lane;
    const int shift = lane * DPL + min_disp;
    int L[DPL];
    int m = 0;
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    // the census words of this pixel and of the two after it: a step's loads are issued two steps ahead of their use
    uint32_t cl, cr[DPL], cla = 0, cra[DPL] = {};
    int xa = x, ya = y;
    sgm_advance(&xa, &ya, dx, dy, W);
    sgm_load_census<DPL>(cenL, cenR, (size_t)y * W, x, shift, vzero, &cl, cr);
    if (steps > 1) sgm_load_census<DPL>(cenL, cenR, (size_t)ya * W, xa, shift, vzero, &cla, cra);
    for (int t = 0; t < steps; ++t) {
        int xb = xa, yb = ya;
        sgm_advance(&xb, &yb, dx, dy, W);
        uint32_t clb = 0, crb[DPL] = {};
        if (t + 2 < steps) sgm_load_census<DPL>(cenL, cenR, (size_t)yb * W, xb, shift, vzero, &clb, crb);

        const bool fresh = t == 0 || (dx > 0 && x == 0) || (dx < 0 && x == W - 1);  // p - r lies outside the image
        int C[DPL];
#pragma unroll
        for (int k = 0; k < DPL; ++k) C[k] = __popc(cl ^ cr[k]);
        if (fresh) {
#pragma unroll
            for (int k = 0; k < DPL; ++k) L[k] = C[k];
        } else {
            const int below = sgm_dpp<0x138, 0xf>(kSgmDropped, L[DPL - 1]);  // wave_shr:1 -- lane l - 1's last: L(d - 1) of k = 0
            const int above = sgm_dpp<0x130, 0xf>(kSgmDropped, L[0]);        // wave_shl:1 -- lane l + 1's first: L(d + 1) of the last k
            int N[DPL];
#pragma unroll
            for (int k = 0; k < DPL; ++k) {
                const int a = k == 0 ? below : L[k - 1], b = k == DPL - 1 ? above : L[k + 1];
                N[k] = C[k] + min(min(L[k], min(a, b) + p1), m + p2) - m;
            }
#pragma unroll
            for (int k = 0; k < DPL; ++k) L[k] = N[k];
        }
        int lo = L[0];
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            lo = min(lo, L[k]);
            word |= (uint32_t)L[k] << (8 * k);
        }
        out[((size_t)y * W + x) * 64] = (Pack)word;  // (64 Packs = D bytes a pixel)
        m = sgm_wave_min(lo);
        x = xa;
        y = ya;
        xa = xb;
        ya = yb;
        cl = cla;
        cla = clb;
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            cr[k] = cra[k];
            cra[k] = crb[k];
        }
    }
    (void)D;
}

// NP: the number of path volumes, 4 or 8 -- a constant, so that a pixel's loads are all issued before the first is used
template <int DPL, int NP>
static __global__ __launch_bounds__(256) void sgm_wta(const uint8_t* __restrict__ vol, size_t vol_stride, int W, int min_disp,
                                                      float uniqueness, uint16_t* __restrict__ lmap, uint32_t* __restrict__ rcand) {
    constexpr int D = 64 * DPL;
    using Pack = typename SgmPack<DPL>::type;
    // candidate i of the tile is for column x0 - (D - 1) - min_disp + i of the right map
    __shared__ uint32_t cand[kSgmTile + D];
    const int y = (int)blockIdx.y, x0 = (int)blockIdx.x * kSgmTile;
    for (int i = (int)threadIdx.x; i < kSgmTile + D; i += 256) cand[i] = kSgmNoCandidate;
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d0 = lane * DPL;
    // a wave takes pixels wave, wave + 4, ... of the tile, four at a time so that their 4 * NP loads are in flight together
    for (int jj = wave; jj < kSgmTile && x0 + jj < W; jj += 16) {
        int S[4][DPL] = {};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = jj + 4 * u;
            if (x0 + j >= W) break;
            const size_t pix = (size_t)y * W + (x0 + j);
            uint32_t word[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) word[p] = reinterpret_cast<const Pack*>(vol + (size_t)p * vol_stride)[pix * 64 + lane];
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int k = 0; k < DPL; ++k) S[u][k] += (int)((word[p] >> (8 * k)) & 0xffu);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = jj + 4 * u;
            if (x0 + j >= W) break;
            const size_t pix = (size_t)y * W + (x0 + j);
            int best = (S[u][0] << 8) | d0;
#pragma unroll
            for (int k = 1; k < DPL; ++k) best = min(best, (S[u][k] << 8) | (d0 + k));
            best = sgm_wave_min(best);  // the smallest S, and of those the smallest d
            const int s1 = best >> 8, dl = best & 0xff;
            int second = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < DPL; ++k) {
                const int gap = d0 + k - dl;
                if (gap > 1 || gap < -1) second = min(second, S[u][k]);
            }
            second = sgm_wave_min(second);
            if (lane == 0) lmap[pix] = (uniqueness * (float)second < (float)s1) ? kSgmInvalid : (uint16_t)dl;
#pragma unroll
            for (int k = 0; k < DPL; ++k) atomicMin(&cand[j + (D - 1) - (d0 + k)], (uint32_t)((S[u][k] << 8) | (d0 + k)));
        }
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < kSgmTile + D - 1; i += 256) {
        const int xp = x0 - (D - 1) - min_disp + i;
        const uint32_t v = cand[i];
        if (xp >= 0 && xp < W && v != kSgmNoCandidate) atomicMin(&rcand[(size_t)y * W + xp], v);
    }
}

__device__ __forceinline__ uint16_t sgm_left_at(const uint16_t* __restrict__ lmap, const uint32_t* __restrict__, size_t i) { return lmap[i]; }
__device__ __forceinline__ uint16_t sgm_right_at(const uint16_t* __restrict__, const uint32_t* __restrict__ rcand, size_t i) {
    const uint32_t v = rcand[i];
    return v == kSgmNoCandidate ? (uint16_t)0 : (uint16_t)(v & 0xffu);
}

// the 3 x 3 median of a map at (y, x); the outermost rows and columns, and a map too small for a window, as they are
template <bool RIGHT>
__device__ __forceinline__ int sgm_median(const uint16_t* __restrict__ lmap, const uint32_t* __restrict__ rcand, int W, int H, int y, int x) {
    auto at = [&](size_t i) { return (int)(RIGHT ? sgm_right_at(lmap, rcand, i) : sgm_left_at(lmap, rcand, i)); };
    const size_t c = (size_t)y * W + x;
    if (y == 0 || x == 0 || y >= H - 1 || x >= W - 1) return at(c);
    int v[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) v[j * 3 + i] = at(c + (size_t)j * W + i - W - 1);
    // odd-even transposition sort of nine
#pragma unroll
    for (int round = 0; round < 9; ++round) {
#pragma unroll
        for (int i = round & 1; i + 1 < 9; i += 2) {
            const int lo = min(v[i], v[i + 1]), hi = max(v[i], v[i + 1]);
            v[i] = lo;
            v[i + 1] = hi;
        }
    }
    return v[4];
}

static __global__ __launch_bounds__(256) void sgm_tail(const uint16_t* __restrict__ lmap, const uint32_t* __restrict__ rcand, int W, int H,
                                                       int min_disp, int lr_max_diff, uint8_t* __restrict__ dst) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int d = sgm_median<false>(lmap, rcand, W, H, y, x);
    bool valid = d != (int)kSgmInvalid;
    if (valid && lr_max_diff >= 0) {
        const int k = x - (d + min_disp);
        valid = false;
        if (k >= 0) {
            const int gap = sgm_median<true>(lmap, rcand, W, H, y, k) - d;
            valid = (gap < 0 ? -gap : gap) <= lr_max_diff;
        }
    }
    dst[(size_t)y * W + x] = valid ? (uint8_t)(d + min_disp) : (uint8_t)(min_disp - 1);
}

static __global__ __launch_bounds__(256) void sgm_sums(const uint8_t* __restrict__ vol, size_t vol_stride, int npaths, size_t count,
                                                       uint16_t* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    int s = 0;
    for (int p = 0; p < npaths; ++p) s += vol[(size_t)p * vol_stride + i];
    dst[i] = (uint16_t)s;
}

struct DisparityQ {
    float q00, q03, q11, q13, q23, q32, q33;
};

// T: the colour channel's type (uint8_t, uint16_t), k: its full scale
template <class T>
static __global__ __launch_bounds__(256) void disparity_points(const uint8_t* __restrict__ disp, const T* __restrict__ color, int W,
                                                               int64_t count, DisparityQ q, float k, float* __restrict__ points,
                                                               float* __restrict__ colors) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int v = (int)(i / W), u = (int)(i % W);
    const float d = (float)disp[i];
    const float w = q.q32 * d + q.q33;
    const float r = (float)(1.0 / (double)w);
    points[i * 3 + 0] = (q.q00 * (float)u + q.q03) * r;
    points[i * 3 + 1] = (q.q11 * (float)v + q.q13) * r;
    points[i * 3 + 2] = q.q23 * r;
#pragma unroll
    for (int c = 0; c < 3; ++c) colors[i * 3 + c] = (float)color[i * 3 + c] / k;
}

}  // namespace mi
