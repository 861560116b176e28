// image_kernels.h -- geometry::Image / geometry::RGBDImage processing: separable filters, the fused pyramid level, the
// bilateral filter, downsampling, the conversions between pixel formats, transpose and the flips (image.cu,
// image_factory.cu, rgbdimage_factory.cu).  The contract is in include/mi_icp.h ("image"); tests/image_exact.py
// restates it in numpy.  All arithmetic is fp32 in the order the contract writes it, unfused (the library is built with
// -ffp-contract=off) except where fmaf is written: the filter taps and the three-channel intensity, which the
// reference's own byte vectors pin (tests/golden/reference_tests.json).  csrc/odometry.h keeps its own od_filter3 /
// od_downsample, which compute the same words (Gaussian3 and the Sobel taps are powers of two: exact products).
//
// SEPARABLE FILTER (img_filter).  A workgroup of four waves writes a tile of 64 x 16 pixels: a wave's 64 lanes are 64
// consecutive x (256-byte rows on both the global and the LDS side, one bank per lane).  It first puts the row sums
// (the horizontal pass, edge clamps on the global loads) of its 16 rows plus `half` halo rows above and below into LDS
// -- at most 64 x (16 + 30) floats = 11.5 KiB --, then forms the column sums from LDS: a halo row is the row sum of the
// CLAMPED row, so the vertical clamp needs no index arithmetic in the second pass.  One read and one write of the
// image where the reference's horizontal / transpose / horizontal / transpose makes four of each.
// FUSED PYRAMID LEVEL (img_pyramid_level).  The same tile with Gaussian3: the filtered 64 x 16 values go to a second
// LDS tile and 256 threads write the 32 x 8 means of their 2 x 2 blocks; only the quarter-size image is written.
// BILATERAL (img_bilateral).  A 16 x 16 tile with a halo of `diameter` pixels in LDS ((16 + 62)^2 floats = 23.8 KiB at
// the largest diameter); each lane walks its window in LDS.  The spatial table comes with the kernel arguments and is
// indexed by the loop counters alone, so those reads are wave-uniform scalar loads.  The kernel is bound by the
// exponential: one per tap.  KEPT: the hardware exponential, v_exp_f32 of arg * log2(e) (EXP 1).  expf (EXP 0, the
// library routine: range reduction and a polynomial, about 1 ulp) stays behind mi_icp_debug_image_bilateral so that
// scripts/dev/image_rows.py can time both; DESIGN 4.12 has the figures and says why the hardware path was kept.
// TRANSPOSE goes through a 32 x 32 LDS tile of pixels' bytes so that reads and writes are both along rows.
// No kernel here keeps a per-lane array that is indexed at run time: there is no scratch.  Nothing needs an atomic.
#pragma once
#include "depth_kernels.h"
#include "device_utils.h"

namespace mi {

constexpr int kImgMaxTaps = 31;       // the longest caller-given filter
constexpr int kImgMaxDiameter = 31;   // the largest bilateral radius ("diameter" in the reference)
constexpr int kImgTileW = 64, kImgTileH = 16, kImgThreads = 256;
constexpr int kImgBiTile = 16;
constexpr int kImgTrTile = 32;

struct ImgTaps {
    float dx[kImgMaxTaps], dy[kImgMaxTaps];
    int nx, ny;  // odd; ny = 0: the horizontal pass alone
};

struct ImgTable {
    float g[2 * kImgMaxDiameter + 1];
    int d;
};

__device__ __forceinline__ int img_clamp(int v, int hi) { return min(max(0, v), hi); }

// the horizontal sum of row `ys` at column x: t = 0; t = fmaf(src[clamp(x + i)], k[i + half], t), ascending i: one
// rounding per tap, as the reference's vectors pin it (Filter_Gaussian5, Filter_Gaussian7; mi_icp.h "image")
__device__ __forceinline__ float img_row_sum(const float* __restrict__ row, int x, int w, const float* k, int half) {
    float t = 0.0f;
    for (int i = -half; i <= half; ++i) t = fmaf(row[img_clamp(x + i, w - 1)], k[i + half], t);
    return t;
}

// Image::Filter(dx, dy) / Image::FilterHorizontal(dx) on 1 x float32.  grid (ceil(w / 64), ceil(h / 16))
static __global__ __launch_bounds__(kImgThreads) void img_filter(const float* __restrict__ src, int w, int h, ImgTaps a,
                                                                 float* __restrict__ dst) {
    __shared__ float rows[(kImgTileH + kImgMaxTaps - 1) * kImgTileW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * kImgTileW + lane, y0 = blockIdx.y * kImgTileH;
    const int hx = a.nx / 2;
    if (a.ny == 0) {
        for (int r = wave; r < kImgTileH; r += 4) {
            const int y = y0 + r;
            if (x < w && y < h) dst[(int64_t)y * w + x] = img_row_sum(src + (int64_t)y * w, x, w, a.dx, hx);
        }
        return;
    }
    const int hy = a.ny / 2;
    for (int r = wave; r < kImgTileH + 2 * hy; r += 4) {
        const int ys = img_clamp(y0 + r - hy, h - 1);
        if (x < w) rows[r * kImgTileW + lane] = img_row_sum(src + (int64_t)ys * w, x, w, a.dx, hx);
    }
    __syncthreads();
    for (int r = wave; r < kImgTileH; r += 4) {
        const int y = y0 + r;
        if (x >= w || y >= h) continue;
        float out = 0.0f;
        for (int j = 0; j <= 2 * hy; ++j) out = fmaf(rows[(r + j) * kImgTileW + lane], a.dy[j], out);
        dst[(int64_t)y * w + x] = out;
    }
}

// one level of Image::CreatePyramid with the Gaussian: Downsample(Filter(Gaussian3)) of a 1 x float32 image, bit-equal
// to the two steps.  grid (ceil(w / 64), ceil(h / 16)); dst is (w / 2) x (h / 2)
static __global__ __launch_bounds__(kImgThreads) void img_pyramid_level(const float* __restrict__ src, int w, int h,
                                                                        float* __restrict__ dst) {
    __shared__ float rows[(kImgTileH + 2) * kImgTileW];
    __shared__ float filt[kImgTileH * kImgTileW];
    const float g0 = 0.25f, g1 = 0.5f, g2 = 0.25f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * kImgTileW + lane, y0 = blockIdx.y * kImgTileH;
    for (int r = wave; r < kImgTileH + 2; r += 4) {
        const int ys = img_clamp(y0 + r - 1, h - 1);
        if (x < w) {
            const float* row = src + (int64_t)ys * w;
            float t = 0.0f;
            t = fmaf(row[img_clamp(x - 1, w - 1)], g0, t);
            t = fmaf(row[x], g1, t);
            t = fmaf(row[img_clamp(x + 1, w - 1)], g2, t);
            rows[r * kImgTileW + lane] = t;
        }
    }
    __syncthreads();
    for (int r = wave; r < kImgTileH; r += 4) {
        if (x >= w || y0 + r >= h) continue;
        float out = 0.0f;
        out = fmaf(rows[r * kImgTileW + lane], g0, out);
        out = fmaf(rows[(r + 1) * kImgTileW + lane], g1, out);
        out = fmaf(rows[(r + 2) * kImgTileW + lane], g2, out);
        filt[r * kImgTileW + lane] = out;
    }
    __syncthreads();
    const int hw = w / 2, hh = h / 2;
    const int ox = threadIdx.x & 31, oy = threadIdx.x >> 5;  // 32 x 8 outputs
    const int X = blockIdx.x * (kImgTileW / 2) + ox, Y = blockIdx.y * (kImgTileH / 2) + oy;
    if (X >= hw || Y >= hh) return;  // (2X + 1 < w and 2Y + 1 < h: all four were written)
    const float* p = filt + (2 * oy) * kImgTileW + 2 * ox;
    dst[(int64_t)Y * hw + X] = (((p[0] + p[1]) + p[kImgTileW]) + p[kImgTileW + 1]) / 4.0f;
}

// exp(arg), arg <= 0 or NaN.  EXP 1: v_exp_f32 (2^x) of arg * log2(e); EXP 0: expf
template <int EXP>
__device__ __forceinline__ float img_exp(float arg) {
    if (EXP == 1) return __builtin_amdgcn_exp2f(arg * 1.44269504088896341f);
    return expf(arg);
}

// Image::BilateralFilter on 1 x float32, taps clamped to the image.  grid (ceil(w / 16), ceil(h / 16)), dynamic LDS
// (16 + 2 d)^2 floats
template <int EXP>
__global__ __launch_bounds__(kImgThreads) void img_bilateral(const float* __restrict__ src, int w, int h, ImgTable t,
                                                             float sigma_color, float* __restrict__ dst) {
    extern __shared__ float tile[];
    const int d = t.d, side = kImgBiTile + 2 * d;
    const int x0 = blockIdx.x * kImgBiTile, y0 = blockIdx.y * kImgBiTile;
    for (int i = threadIdx.x; i < side * side; i += kImgThreads) {
        const int ty = i / side, tx = i - ty * side;
        tile[i] = src[(int64_t)img_clamp(y0 + ty - d, h - 1) * w + img_clamp(x0 + tx - d, w - 1)];
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    const float center = tile[(ly + d) * side + lx + d];
    const float denom = (2.0f * sigma_color) * sigma_color;
    float filtered = 0.0f, total = 0.0f;
    for (int dy = 0; dy <= 2 * d; ++dy) {
        const float gy = t.g[dy];
        const float* row = tile + (ly + dy) * side + lx;
        for (int dx = 0; dx <= 2 * d; ++dx) {
            const float cur = row[dx];
            const float c = center - cur;
            const float wgt = (gy * t.g[dx]) * img_exp<EXP>(-(c * c) / denom);
            filtered = filtered + wgt * cur;
            total = total + wgt;
        }
    }
    dst[(int64_t)y * w + x] = filtered / total;
}

// Image::Downsample, 1 x float32
static __global__ __launch_bounds__(256) void img_downsample_f32(const float* __restrict__ src, int w, int hw, int64_t count,
                                                                 float* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const int64_t y = idx / hw, x = idx - y * hw;
    const float* p = src + (y * 2) * w + x * 2;
    dst[idx] = (((p[0] + p[1]) + p[w]) + p[w + 1]) / 4.0f;
}

// Image::Downsample, 3 x uint8: the integer mean of every channel (one thread per output byte)
static __global__ __launch_bounds__(256) void img_downsample_rgb8(const uint8_t* __restrict__ src, int w, int hw, int64_t count,
                                                                  uint8_t* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count * 3) return;
    const int64_t pix = idx / 3, ch = idx - pix * 3;
    const int64_t y = pix / hw, x = pix - y * hw;
    const uint8_t* p = src + ((y * 2) * w + x * 2) * 3 + ch;
    const int sum = (int)p[0] + (int)p[3] + (int)p[(int64_t)w * 3] + (int)p[(int64_t)w * 3 + 3];
    dst[idx] = (uint8_t)(sum / 4);
}

// float -> unsigned by truncation, saturating; NaN -> 0
__device__ __forceinline__ uint32_t img_sat(float v, float top) {
    if (!(v > 0.0f)) return 0u;
    if (v >= top) return (uint32_t)top;
    return (uint32_t)v;
}

struct ImgFormat {
    int channels, bytes;   // per pixel, per channel
    float w0, w1, w2;      // the colour weights
    float denom;
};

// the value make_gray_image_functor forms before the conversion to the output type: one channel value * denom, three
// channels fmaf(w2, v2, fmaf(w0, v0, w1 * v1)) * denom -- the contraction the reference's vectors pin
// (CreateFloatImage_3_1 / 3_2 / 3_4; both weight sets: the reference compiles one expression) --, anything else 0
__device__ __forceinline__ float img_intensity(const uint8_t* __restrict__ src, int64_t idx, const ImgFormat& f) {
    float v[3] = {0.0f, 0.0f, 0.0f};
    const int n = f.channels == 3 ? 3 : (f.channels == 1 ? 1 : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= n) break;
        const int64_t e = idx * f.channels + k;
        if (f.bytes == 1) v[k] = (float)src[e];
        else if (f.bytes == 2) v[k] = (float)reinterpret_cast<const uint16_t*>(src)[e];
        else if (f.bytes == 4) v[k] = reinterpret_cast<const float*>(src)[e];
    }
    if (n == 1) return v[0] * f.denom;
    if (n == 3) return fmaf(f.w2, v[2], fmaf(f.w0, v[0], f.w1 * v[1])) * f.denom;
    return 0.0f;
}

// Image::CreateFloatImage; DEPTH: ConvertDepthToFloatImage's depth_metres (depth_kernels.h) in the same pass
template <bool DEPTH>
__global__ __launch_bounds__(256) void img_to_float(const uint8_t* __restrict__ src, int64_t count, ImgFormat f, float recip,
                                                    float trunc, float* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    float v = img_intensity(src, idx, f);
    if (DEPTH) v = depth_metres(v, recip, trunc);
    dst[idx] = v;
}

// Image::CreateGrayImage
static __global__ __launch_bounds__(256) void img_to_gray(const uint8_t* __restrict__ src, int64_t count, ImgFormat f,
                                                          uint8_t* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    dst[idx] = (uint8_t)img_sat(img_intensity(src, idx, f), 255.0f);
}

// Image::CreateImageFromFloatImage<uint8_t> (value * 255) and <uint16_t> (the value)
template <class T>
__global__ __launch_bounds__(256) void img_from_float(const float* __restrict__ src, int64_t count, T* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    dst[idx] = sizeof(T) == 1 ? (T)img_sat(src[idx] * 255.0f, 255.0f) : (T)img_sat(src[idx], 65535.0f);
}

// Image::LinearTransform in place: float scale * f + offset; uint8 (uint8)(scale * (float)f + offset), saturating
template <class T>
__global__ __launch_bounds__(256) void img_linear(T* __restrict__ data, int64_t count, float scale, float offset) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const float v = scale * (float)data[idx] + offset;
    data[idx] = sizeof(T) == 1 ? (T)img_sat(v, 255.0f) : (T)v;
}

// Image::ClipIntensity in place: fmaxf(fminf(max_, f), min_) -- the device's min / max, which drop a NaN operand, so a
// NaN pixel becomes max_ (as in the reference)
static __global__ __launch_bounds__(256) void img_clip(float* __restrict__ data, int64_t count, float lo, float hi) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    data[idx] = fmaxf(fminf(hi, data[idx]), lo);
}

// the SUN and NYU depth encodings (rgbdimage_factory.cu), uint16 to uint16
template <int NYU>
__global__ __launch_bounds__(256) void img_depth_format(const uint16_t* __restrict__ src, int64_t count, uint16_t* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const uint32_t d = src[idx];
    if (!NYU) {
        dst[idx] = (uint16_t)((d >> 3) | (d << 13));
        return;
    }
    const uint32_t s = ((d & 0xffu) << 8) | (d >> 8);
    const float xx = (float)(351.3 / (1092.5 - (double)s));
    if (xx <= 0.0f) {
        dst[idx] = 0;
        return;
    }
    const double r = floor((double)xx * 1000.0 + 0.5);
    dst[idx] = (uint16_t)(r >= 65535.0 ? 65535u : (uint32_t)r);   // (xx > 0: r >= 0; xx is never NaN: 1092.5 - s is never 0)
}

// Image::FlipVertical (OP 0) / FlipHorizontal (OP 1): whole pixels of bpp bytes, one thread per byte
template <int OP>
__global__ __launch_bounds__(256) void img_flip(const uint8_t* __restrict__ src, int w, int h, int bpp, uint8_t* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t line = (int64_t)w * bpp;
    if (idx >= line * h) return;
    const int64_t y = idx / line, off = idx - y * line;
    const int64_t x = off / bpp, b = off - x * bpp;
    const int64_t sy = OP == 0 ? h - 1 - y : y, sx = OP == 0 ? x : w - 1 - x;
    dst[idx] = src[sy * line + sx * bpp + b];
}

// Image::Transpose: a 32 x 32 tile of pixels through LDS, rows on both sides.  A pixel is `upp` units of U (bytes, or
// dwords where the pixel is a multiple of four bytes).  grid (ceil(w / 32), ceil(h / 32)), dynamic LDS
// 32 * img_tr_stride(upp) units (a tile row is padded by one unit: the transposed read of one-unit pixels then touches
// 32 different banks); dst is h pixels wide, w high
__host__ __device__ inline int img_tr_stride(int upp) { return kImgTrTile * upp + 1; }

template <class U>
__global__ __launch_bounds__(kImgThreads) void img_transpose(const U* __restrict__ src, int w, int h, int upp, U* __restrict__ dst) {
    extern __shared__ float tile[];
    U* t = reinterpret_cast<U*>(tile);
    const int stride = img_tr_stride(upp);
    const int x0 = blockIdx.x * kImgTrTile, y0 = blockIdx.y * kImgTrTile;
    const int tw = min(kImgTrTile, w - x0), th = min(kImgTrTile, h - y0);
    const int in_line = tw * upp;      // units of a tile row on the source side
    for (int i = threadIdx.x; i < in_line * th; i += kImgThreads) {
        const int r = i / in_line, o = i - r * in_line;
        t[r * stride + o] = src[((int64_t)(y0 + r) * w + x0) * upp + o];
    }
    __syncthreads();
    const int out_line = th * upp;     // the transposed tile's row: th pixels
    for (int i = threadIdx.x; i < out_line * tw; i += kImgThreads) {
        const int r = i / out_line, o = i - r * out_line;   // r: the source column
        const int p = o / upp, b = o - p * upp;             // p: the source row
        dst[((int64_t)(x0 + r) * h + y0) * upp + o] = t[p * stride + r * upp + b];
    }
}

}  // namespace mi
