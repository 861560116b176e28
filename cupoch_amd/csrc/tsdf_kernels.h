// tsdf_kernels.h -- integration::UniformTSDFVolume (integration/uniform_tsdfvolume.cu, integrate_functor.h,
// geometry/image_factory.cu:32-48,136-165): Integrate, Raycast, ExtractPointCloud, ExtractVoxelPointCloud.
// include/mi_icp.h holds the numeric contract (operation order); everything below is fp32 with unfused products.
//
// The volume is five planes of resolution^3 floats -- tsdf, weight and (only with a colour type) three colour planes
// -- indexed x*res*res + y*res + z, z fastest.  The reference keeps an array of 20-byte voxels.
// TsdfPlanes, tsdf_reset, tsdf_update_voxel (the per-voxel rule) and the small tsdf_blend_color / tsdf_normalize /
// tsdf_grey below are also ScalableTSDFVolume's (scalable_tsdf_kernels.h): each stands here once.
//   tsdf_multiplier   the depth -> camera-distance multiplier image, once per intrinsic (cached on the volume)
//   tsdf_integrate    a wave takes 64 consecutive z of one (x, y) column and hands each voxel's camera point to
//                     tsdf_update_voxel: whether a voxel is updated is decided from its projection and one depth
//                     gather; only then are its planes loaded and stored (8 bytes each way without colour, 20 with).
//                     A wave whose z-span lies behind the camera or beside the image by a margin that covers every
//                     rounding of the per-voxel arithmetic leaves before any of it.
//   tsdf_raycast      one lane per pixel, an 8x8 pixel tile per wave, so that neighbouring rays gather neighbouring
//                     voxels; one launch covers every level of a camera pyramid (TsdfRayLevel), a workgroup finds its
//                     level from its index.  Writes NaN for an invalid pixel; finite_flags + scan + select_gather
//                     (select.h) over the concatenated pixels remove those when asked, tsdf_level_ends reads the
//                     levels' counts from the scan.
//   tsdf_cloud_count / tsdf_cloud_gather   ExtractPointCloud: per interior voxel the number of its +x, +y, +z edges
//                     that cross zero; after the scan the gather recomputes the survivors' points, colours and
//                     normals (6 x 8 tsdf gathers each, GetNormalAt).
//   tsdf_voxel_flags / tsdf_voxel_gather   ExtractVoxelPointCloud: the valid voxels, ascending.
// No kernel here keeps an array in registers that is indexed at run time: none uses scratch memory (tsdf_raycast's table
// of levels is a kernel argument read through a workgroup-uniform index, i.e. scalar loads).
#pragma once
#include "device_utils.h"
#include "grid_rules.h"

namespace mi {

constexpr int kTsdfNoColor = 0, kTsdfRGB8 = 1, kTsdfGray32 = 2;

// the planes of a volume or of a pool of units; plane k of the colour starts at color + k * stride
struct TsdfPlanes {
    float* tsdf;
    float* weight;
    float* color;    // three planes of `stride` floats, or null (NoColor)
    int64_t stride;  // floats in a plane
    int color_type;
};

struct TsdfVol {
    TsdfPlanes p;  // stride = res^3
    int res, h_res;
    float voxel_length, half;  // half = 0.5 * voxel_length
    float origin[3];
};

// voxels [first, first + count) back to tsdf 0, weight 0, colour (1, 1, 1)
static __global__ __launch_bounds__(256) void tsdf_reset(TsdfPlanes p, int64_t first, int64_t count) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    const int64_t i = first + j;
    p.tsdf[i] = 0.0f;
    p.weight[i] = 0.0f;
    if (p.color) {
        p.color[i] = 1.0f;
        p.color[p.stride + i] = 1.0f;
        p.color[2 * p.stride + i] = 1.0f;
    }
}

// Image::CreateDepthToCameraDistanceMultiplierFloatImage: sqrtf(xx*xx + yy*yy + 1), xx = (j - cx) * (1/fx)
static __global__ __launch_bounds__(256) void tsdf_multiplier(float* __restrict__ out, int width, int height, float cx, float cy,
                                                             float inv_fx, float inv_fy) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)width * height) return;
    const int i = (int)(idx / width), j = (int)(idx % width);
    const float xx = ((float)j - cx) * inv_fx, yy = ((float)i - cy) * inv_fy;
    out[idx] = sqrtf((xx * xx + yy * yy) + 1.0f);
}

struct TsdfIntegrate {
    float E[3][4];  // extrinsic, rows 0..2
    float D[3];     // (voxel_length * extrinsic)[r][2]
    float fx, fy, cx, cy, safe_w, safe_h, sdf_trunc, sdf_trunc_inv;
    int width, height;
    const float* depth;
    const float* mult;
    const void* color;  // uint8 x 3 (RGB8) or float (Gray32)
    // the span test: 0 switches it off (intrinsics too large for its error bound)
    int cull;
    float k_left, k_right, k_top, k_bottom;  // cx + 1.5, width + 0.5 - cx, cy + 1.5, height + 0.5 - cy
};

// THE PER-VOXEL RULE of both volumes (integrate_functor.h): voxel i of the planes, whose centre is the camera point
// (X, Y, Z), takes the frame's observation -- project, gather the depth, truncate, running mean of tsdf and of the
// three colour planes, weight + 1 -- or is left as it is.  It knows nothing of the volume that calls it.
// What the two volumes do NOT share, because the reference's own two classes differ there: tsdf_at / stsdf_at (and
// GetNormalAt's half_gap, a double in the uniform volume, a float in the scalable one), the template-axis
// tsdf_cloud_emit against the run-time-axis stsdf_cloud_emit, and tsdf_raycast (the scalable volume has none).
__device__ __forceinline__ void tsdf_update_voxel(const TsdfPlanes& p, int64_t i, float X, float Y, float Z, const TsdfIntegrate& a) {
    if (Z <= 0.0f) return;
    const float u_f = (X * a.fx / Z + a.cx) + 0.5f;
    const float v_f = (Y * a.fy / Z + a.cy) + 0.5f;
    if (!(u_f >= 0.0001f && u_f < a.safe_w && v_f >= 0.0001f && v_f < a.safe_h)) return;
    // 0.0001 <= u_f < safe_w <= width: the pixel is inside the image
    const int pu = (int)floorf(u_f), pv = (int)floorf(v_f);
    const int64_t pix = (int64_t)pv * a.width + pu;
    const float d = a.depth[pix];
    if (d <= 0.0f) return;
    const float sdf = (d - Z) * a.mult[pix];
    if (!(sdf > -a.sdf_trunc)) return;
    const float t = fminf(1.0f, sdf * a.sdf_trunc_inv);
    const float w = p.weight[i], w1 = w + 1.0f;
    p.tsdf[i] = (p.tsdf[i] * w + t) / w1;
    if (p.color_type == kTsdfRGB8) {
        const uint8_t* rgb = (const uint8_t*)a.color + pix * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) p.color[k * p.stride + i] = (p.color[k * p.stride + i] * w + (float)rgb[k]) / w1;
    } else if (p.color_type == kTsdfGray32) {
        const float g = ((const float*)a.color)[pix];
#pragma unroll
        for (int k = 0; k < 3; ++k) p.color[k * p.stride + i] = (p.color[k * p.stride + i] * w + g) / w1;
    }
    p.weight[i] = w1;
}

// X*fx + k*Z at one end of a span (the quantity whose sign says on which side of an image edge, moved out by one
// pixel, the point projects)
__device__ __forceinline__ float tsdf_side(float X, float f, float k, float Z) { return X * f + k * Z; }

static __global__ __launch_bounds__(256) void tsdf_integrate(TsdfVol v, TsdfIntegrate a, int zchunks) {
    const int col = (int)(blockIdx.x / (unsigned)zchunks);  // x * res + y
    const int zc = (int)(blockIdx.x % (unsigned)zchunks);
    const int wave_z0 = zc * 256 + (int)(threadIdx.x & ~63u);
    if (wave_z0 >= v.res) return;
    const int xi = col / v.res - v.h_res, yi = col % v.res - v.h_res;
    const float px = (v.half + v.voxel_length * (float)xi) + v.origin[0];
    const float py = (v.half + v.voxel_length * (float)yi) + v.origin[1];
    const float pz = v.half + v.origin[2];
    const float X0 = ((a.E[0][0] * px + a.E[0][1] * py) + a.E[0][2] * pz) + a.E[0][3];
    const float Y0 = ((a.E[1][0] * px + a.E[1][1] * py) + a.E[1][2] * pz) + a.E[1][3];
    const float Z0 = ((a.E[2][0] * px + a.E[2][1] * py) + a.E[2][2] * pz) + a.E[2][3];

    if (a.cull) {
        // The camera points of this wave's voxels lie, up to rounding, on the segment between those of its first and
        // last z.  err bounds the distance of any computed coordinate from that segment (each is two roundings of
        // values no larger than 2 s, s the largest coordinate of the two ends and of the column's z = 0 point; 2^-20 s is
        // several times that) and the error of the side expressions below
        // (products with fx, k scale it by their size: the factor kk).  A voxel is updated only if its computed Z > 0
        // and its computed pixel lies inside the image.  If at both ends Z < -err, every computed Z is negative.  If
        // at both ends X*fx + (cx + 1.5)*Z < -err*kk, then for every voxel with computed Z > 0 the exact quotient
        // X*fx/Z + cx + 0.5 of its computed coordinates is below -1, and the three roundings of the computed u_f
        // (relative 2^-24 each, cx and the image at most 2^16: the host checks) cannot lift it to 0.0001.  The other
        // three edges likewise.  A NaN anywhere makes every comparison false: the wave goes on.
        const float zlo = (float)(wave_z0 - v.h_res), zhi = (float)(min(wave_z0 + 63, v.res - 1) - v.h_res);
        const float Xa = X0 + zlo * a.D[0], Ya = Y0 + zlo * a.D[1], Za = Z0 + zlo * a.D[2];
        const float Xb = X0 + zhi * a.D[0], Yb = Y0 + zhi * a.D[1], Zb = Z0 + zhi * a.D[2];
        const float s = fmaxf(fmaxf(fmaxf(fabsf(Xa), fabsf(Xb)), fmaxf(fmaxf(fabsf(Ya), fabsf(Yb)), fmaxf(fabsf(Za), fabsf(Zb)))),
                              fmaxf(fabsf(X0), fmaxf(fabsf(Y0), fabsf(Z0))));
        const float err = s * 9.5367431640625e-7f;  // 2^-20
        const float kx = (fabsf(a.fx) + fmaxf(fabsf(a.k_left), fabsf(a.k_right))) * 4.0f;
        const float ky = (fabsf(a.fy) + fmaxf(fabsf(a.k_top), fabsf(a.k_bottom))) * 4.0f;
        const bool behind = Za < -err && Zb < -err;
        const bool left = tsdf_side(Xa, a.fx, a.k_left, Za) < -err * kx && tsdf_side(Xb, a.fx, a.k_left, Zb) < -err * kx;
        const bool right = tsdf_side(Xa, a.fx, -a.k_right, Za) > err * kx && tsdf_side(Xb, a.fx, -a.k_right, Zb) > err * kx;
        const bool top = tsdf_side(Ya, a.fy, a.k_top, Za) < -err * ky && tsdf_side(Yb, a.fy, a.k_top, Zb) < -err * ky;
        const bool bottom = tsdf_side(Ya, a.fy, -a.k_bottom, Za) > err * ky && tsdf_side(Yb, a.fy, -a.k_bottom, Zb) > err * ky;
        if (behind || left || right || top || bottom) return;
    }

    const int z = zc * 256 + (int)threadIdx.x;
    if (z >= v.res) return;
    const float zf = (float)(z - v.h_res);
    const float X = X0 + zf * a.D[0], Y = Y0 + zf * a.D[1], Z = Z0 + zf * a.D[2];
    tsdf_update_voxel(v.p, (int64_t)col * v.res + z, X, Y, Z, a);
}

// ---- extraction -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool tsdf_valid(float w, float f) { return w != 0.0f && f < 0.98f && f >= -0.98f; }

// colour plane k of a surface point between voxels i0 and i1 (|tsdf| r0 and r1, rs their sum), RGB8 scaled to [0, 1]
__device__ __forceinline__ float tsdf_blend_color(const TsdfPlanes& p, int k, int64_t i0, int64_t i1, float r0, float r1, float rs) {
    const float c = (p.color[k * p.stride + i0] * r1 + p.color[k * p.stride + i1] * r0) / rs;
    return p.color_type == kTsdfRGB8 ? c / 255.0f : c;
}

// a normal to unit length; a zero one stays
__device__ __forceinline__ void tsdf_normalize(float n[3]) {
    const float zz = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (zz > 0.0f) {
        const float len = sqrtf(zz);
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
    }
}

// ExtractVoxelPointCloud's colour of a voxel
__device__ __forceinline__ float tsdf_grey(float tsdf) { return (float)(((double)tsdf + 1.0) * 0.5); }

static __global__ __launch_bounds__(256) void tsdf_voxel_flags(TsdfVol v, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= v.p.stride) return;
    flags[i] = tsdf_valid(v.p.weight[i], v.p.tsdf[i]) ? 1u : 0u;
}

static __global__ __launch_bounds__(256) void tsdf_voxel_gather(TsdfVol v, const uint32_t* __restrict__ flags,
                                                               const uint32_t* __restrict__ pos, float* __restrict__ oxyz,
                                                               float* __restrict__ ocol) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= v.p.stride || !flags[i]) return;
    const int64_t p = pos[i];
    const int res2 = v.res * v.res;
    const int x = (int)(i / res2), yz = (int)(i % res2), y = yz / v.res, z = yz % v.res;
    oxyz[p * 3] = (v.half + v.voxel_length * (float)(x - v.h_res)) + v.origin[0];
    oxyz[p * 3 + 1] = (v.half + v.voxel_length * (float)(y - v.h_res)) + v.origin[1];
    oxyz[p * 3 + 2] = (v.half + v.voxel_length * (float)(z - v.h_res)) + v.origin[2];
    const float c = tsdf_grey(v.p.tsdf[i]);
    ocol[p * 3] = c;
    ocol[p * 3 + 1] = c;
    ocol[p * 3 + 2] = c;
}

// interior voxel number j of (res-2)^3 -> (x, y, z), each in [1, res-2]
__device__ __forceinline__ void tsdf_interior(int64_t j, int res, int* x, int* y, int* z) {
    const int m = res - 2;
    *x = (int)(j / ((int64_t)m * m)) + 1;
    const int yz = (int)(j % ((int64_t)m * m));
    *y = yz / m + 1;
    *z = yz % m + 1;
}

// does the edge from voxel i0 (valid, tsdf f0) to its neighbour at +stride along an axis with coordinate c cross zero?
__device__ __forceinline__ bool tsdf_edge(const TsdfVol& v, int64_t i0, float f0, int c, int64_t stride, float* f1) {
    if (!(c + 1 < v.res - 1)) return false;
    *f1 = v.p.tsdf[i0 + stride];
    return tsdf_valid(v.p.weight[i0 + stride], *f1) && f0 * *f1 < 0.0f;
}

static __global__ __launch_bounds__(256) void tsdf_cloud_count(TsdfVol v, int64_t ninner, uint32_t* __restrict__ count) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ninner) return;
    int x, y, z;
    tsdf_interior(j, v.res, &x, &y, &z);
    const int64_t i0 = ((int64_t)x * v.res + y) * v.res + z;
    const float f0 = v.p.tsdf[i0];
    uint32_t cnt = 0;
    if (tsdf_valid(v.p.weight[i0], f0)) {
        float f1;
        cnt += tsdf_edge(v, i0, f0, x, (int64_t)v.res * v.res, &f1) ? 1u : 0u;
        cnt += tsdf_edge(v, i0, f0, y, v.res, &f1) ? 1u : 0u;
        cnt += tsdf_edge(v, i0, f0, z, 1, &f1) ? 1u : 0u;
    }
    count[j] = cnt;
}

// GetTSDFAt: trilinear tsdf at p (grid coordinates from the volume's corner, in metres).  The indices are held inside
// the volume; for the points GetNormalAt asks about they are inside already.
__device__ __forceinline__ float tsdf_at(const TsdfVol& v, float p0, float p1, float p2) {
    const float g0 = p0 / v.voxel_length - 0.5f, g1 = p1 / v.voxel_length - 0.5f, g2 = p2 / v.voxel_length - 0.5f;
    const int top = v.res - 2;
    const int i0 = min(max(floor_int(g0), 0), top), i1 = min(max(floor_int(g1), 0), top),
              i2 = min(max(floor_int(g2), 0), top);
    const float r0 = g0 - (float)i0, r1 = g1 - (float)i1, r2 = g2 - (float)i2;
    const float* __restrict__ T = v.p.tsdf + ((int64_t)i0 * v.res + i1) * v.res + i2;
    const int64_t sx = (int64_t)v.res * v.res, sy = v.res;
    float s = 0.0f;
    s += (1.0f - r0) * (1.0f - r1) * (1.0f - r2) * T[0];
    s += (1.0f - r0) * (1.0f - r1) * r2 * T[1];
    s += (1.0f - r0) * r1 * (1.0f - r2) * T[sy];
    s += (1.0f - r0) * r1 * r2 * T[sy + 1];
    s += r0 * (1.0f - r1) * (1.0f - r2) * T[sx];
    s += r0 * (1.0f - r1) * r2 * T[sx + 1];
    s += r0 * r1 * (1.0f - r2) * T[sx + sy];
    s += r0 * r1 * r2 * T[sx + sy + 1];
    return s;
}

template <int AX>
__device__ __forceinline__ void tsdf_cloud_emit(const TsdfVol& v, int64_t i0, int64_t stride, float f0, float f1, int x, int y,
                                                int z, int64_t p, float* __restrict__ oxyz, float* __restrict__ onrm,
                                                float* __restrict__ ocol) {
    const float r0 = fabsf(f0), r1 = fabsf(f1), rs = r0 + r1;
    float q[3] = {v.half + v.voxel_length * (float)x, v.half + v.voxel_length * (float)y, v.half + v.voxel_length * (float)z};
    const float q1 = q[AX] + v.voxel_length;
    q[AX] = (q[AX] * r1 + q1 * r0) / rs;
    const float hres = (float)v.h_res * v.voxel_length;
#pragma unroll
    for (int k = 0; k < 3; ++k) oxyz[p * 3 + k] = (q[k] + v.origin[k]) - hres;
    if (ocol) {
#pragma unroll
        for (int k = 0; k < 3; ++k) ocol[p * 3 + k] = tsdf_blend_color(v.p, k, i0, i0 + stride, r0, r1, rs);
    }
    // GetNormalAt: half_gap = 0.99 * voxel_length in double, applied to a float
    const double gap = 0.99 * (double)v.voxel_length;
    float n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = (float)((double)q[k] - gap), hi = (float)((double)q[k] + gap);
        const float a = tsdf_at(v, k == 0 ? hi : q[0], k == 1 ? hi : q[1], k == 2 ? hi : q[2]);
        const float b = tsdf_at(v, k == 0 ? lo : q[0], k == 1 ? lo : q[1], k == 2 ? lo : q[2]);
        n[k] = a - b;
    }
    tsdf_normalize(n);
#pragma unroll
    for (int k = 0; k < 3; ++k) onrm[p * 3 + k] = n[k];
}

static __global__ __launch_bounds__(256) void tsdf_cloud_gather(TsdfVol v, int64_t ninner, const uint32_t* __restrict__ count,
                                                               const uint32_t* __restrict__ pos, float* __restrict__ oxyz,
                                                               float* __restrict__ onrm, float* __restrict__ ocol) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ninner || !count[j]) return;
    int x, y, z;
    tsdf_interior(j, v.res, &x, &y, &z);
    const int64_t i0 = ((int64_t)x * v.res + y) * v.res + z;
    const float f0 = v.p.tsdf[i0];
    int64_t p = pos[j];
    float f1;
    const int64_t sx = (int64_t)v.res * v.res, sy = v.res;
    if (tsdf_edge(v, i0, f0, x, sx, &f1)) tsdf_cloud_emit<0>(v, i0, sx, f0, f1, x, y, z, p++, oxyz, onrm, ocol);
    if (tsdf_edge(v, i0, f0, y, sy, &f1)) tsdf_cloud_emit<1>(v, i0, sy, f0, f1, x, y, z, p++, oxyz, onrm, ocol);
    if (tsdf_edge(v, i0, f0, z, 1, &f1)) tsdf_cloud_emit<2>(v, i0, 1, f0, f1, x, y, z, p++, oxyz, onrm, ocol);
}

// ---- raycast --------------------------------------------------------------------------------------------------------
constexpr int kTsdfMaxLevels = 16;  // MI_ICP_TSDF_MAX_LEVELS

// one level of the camera's pyramid (PinholeCameraIntrinsic::CreatePyramidLevel) and where its work and output start
struct TsdfRayLevel {
    float fx, fy, cx, cy;
    int width, height;
    int tiles_x;          // 16 x 16 tiles in a row of this level
    int first_tile;       // the level's first workgroup; an empty level has the next level's
    int64_t first_pixel;  // the level's first pixel in the concatenated output
};

struct TsdfRaycast {
    float R[3][3], t[3];  // camera pose (the inverse of the extrinsic) with the volume's origin taken off t
    float sdf_trunc;
    int levels;
    TsdfRayLevel level[kTsdfMaxLevels];  // read through a workgroup-uniform index: scalar loads of the kernel's arguments
};

__device__ __forceinline__ bool tsdf_inside(int g0, int g1, int g2, int lo, int res) {
    return g0 >= lo && g0 < res - 1 && g1 >= lo && g1 < res - 1 && g2 >= lo && g2 < res - 1;
}

// InterpolateTrilinearly at a point in voxel units, every coordinate in [0, res-1)
__device__ __forceinline__ float tsdf_trilinear(const TsdfVol& v, float p0, float p1, float p2) {
    int i0 = (int)p0, i1 = (int)p1, i2 = (int)p2;
    i0 = (p0 < (float)i0 + 0.5f) ? i0 - 1 : i0;
    i1 = (p1 < (float)i1 + 0.5f) ? i1 - 1 : i1;
    i2 = (p2 < (float)i2 + 0.5f) ? i2 - 1 : i2;
    const float a = p0 - ((float)i0 + 0.5f), b = p1 - ((float)i1 + 0.5f), c = p2 - ((float)i2 + 0.5f);
    const int top = v.res - 2;  // held inside the volume; the callers' range checks put them there already
    i0 = min(max(i0, 0), top);
    i1 = min(max(i1, 0), top);
    i2 = min(max(i2, 0), top);
    const float* __restrict__ T = v.p.tsdf + ((int64_t)i0 * v.res + i1) * v.res + i2;
    const int64_t sx = (int64_t)v.res * v.res, sy = v.res;
    return ((((((T[0] * (1.0f - a) * (1.0f - b) * (1.0f - c) + T[1] * (1.0f - a) * (1.0f - b) * c) +
                T[sy] * (1.0f - a) * b * (1.0f - c)) +
               T[sy + 1] * (1.0f - a) * b * c) +
              T[sx] * a * (1.0f - b) * (1.0f - c)) +
             T[sx + 1] * a * (1.0f - b) * c) +
            T[sx + sy] * a * b * (1.0f - c)) +
           T[sx + sy + 1] * a * b * c;
}

__device__ __forceinline__ void tsdf_store3(float* __restrict__ o, int64_t i, float a, float b, float c) {
    o[i * 3] = a;
    o[i * 3 + 1] = b;
    o[i * 3 + 2] = c;
}

// THE PER-PIXEL RULE of Raycast (include/mi_icp.h): the ray of pixel (x, y) of the camera L, marched through the volume;
// point, normal and colour of its first crossing from positive to negative, else P, N and C stay as they came
__device__ __forceinline__ void tsdf_raycast_pixel(const TsdfVol& v, const TsdfRaycast& a, const TsdfRayLevel& L, int x, int y,
                                                   float (&P)[3], float (&N)[3], float (&C)[3]) {
    const int res = v.res;
    const float vl = v.voxel_length;
    do {
        const float length = (float)res * vl;
        const float ppx = ((float)x - L.cx) / L.fx, ppy = ((float)y - L.cy) / L.fy;
        float d0 = (a.R[0][0] * ppx + a.R[0][1] * ppy) + a.R[0][2];
        float d1 = (a.R[1][0] * ppx + a.R[1][1] * ppy) + a.R[1][2];
        float d2 = (a.R[2][0] * ppx + a.R[2][1] * ppy) + a.R[2][2];
        const float dn = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        if (!(dn > 0.0f)) break;  // zero, or NaN (the reference tests == 0 only; a NaN direction has no ray)
        d0 = d0 / dn;
        d1 = d1 / dn;
        d2 = d2 / dn;
        const float t0 = a.t[0], t1 = a.t[1], t2 = a.t[2];
        // GetMinTime / GetMaxTime: IEEE quotients (a zero direction component gives +-inf or NaN), fmax / fmin return
        // the operand that is not NaN
        const float tmin = fmaxf(fmaxf(((d0 > 0.0f ? 0.0f : length) - t0) / d0, ((d1 > 0.0f ? 0.0f : length) - t1) / d1),
                                 ((d2 > 0.0f ? 0.0f : length) - t2) / d2);
        const float tmax = fminf(fminf(((d0 > 0.0f ? length : 0.0f) - t0) / d0, ((d1 > 0.0f ? length : 0.0f) - t1) / d1),
                                 ((d2 > 0.0f ? length : 0.0f) - t2) / d2);
        float ray_len = fmaxf(tmin, 0.0f);
        if (ray_len >= tmax) break;
        if (!(ray_len < INFINITY)) break;  // (tmax NaN: all three quotients 0/0 -- no ray to march)
        ray_len = ray_len + vl;
        int g0 = floor_int((t0 + d0 * ray_len) / vl) + v.h_res;
        int g1 = floor_int((t1 + d1 * ray_len) / vl) + v.h_res;
        int g2 = floor_int((t2 + d2 * ray_len) / vl) + v.h_res;
        if (!tsdf_inside(g0, g1, g2, 0, res)) break;
        float cur = v.p.tsdf[((int64_t)g0 * res + g1) * res + g2];
        const float max_len = ray_len + length * 1.41421354f;  // sqrt(2.0f)
        const float step = a.sdf_trunc * 0.5f;
        // The march must advance: a step below half an ulp of the ray length would leave ray_len where it is for ever
        // (the reference does not terminate there).  Such a ray is invalid.  ulp grows with ray_len, so the test at the
        // far end covers the whole march; the host bounds the number of steps (length * sqrt(2) / step).
        if (!(step > 0.0f) || !(max_len + step > max_len)) break;
        for (; ray_len < max_len; ray_len = ray_len + step) {
            const float ahead = ray_len + step;
            g0 = floor_int((t0 + d0 * ahead) / vl) + v.h_res;
            g1 = floor_int((t1 + d1 * ahead) / vl) + v.h_res;
            g2 = floor_int((t2 + d2 * ahead) / vl) + v.h_res;
            if (!tsdf_inside(g0, g1, g2, 1, res)) continue;
            const float prev = cur;
            cur = v.p.tsdf[((int64_t)g0 * res + g1) * res + g2];
            if (prev < 0.0f && cur > 0.0f) break;
            if (prev > 0.0f && cur < 0.0f) {
                const float t_star = ray_len - step * prev / (cur - prev);
                const float v0 = t0 + d0 * t_star, v1 = t1 + d1 * t_star, v2 = t2 + d2 * t_star;
                const float hr = (float)v.h_res, hi = (float)(res - 1);
                const float l0 = v0 / vl + hr, l1 = v1 / vl + hr, l2 = v2 / vl + hr;
                if (!(l0 >= 1.0f && l0 < hi && l1 >= 1.0f && l1 < hi && l2 >= 1.0f && l2 < hi)) break;
                if (!(l0 + 1.0f < hi) || !(l0 - 1.0f >= 1.0f)) break;
                const float nx = tsdf_trilinear(v, l0 + 1.0f, l1, l2) - tsdf_trilinear(v, l0 - 1.0f, l1, l2);
                if (!(l1 + 1.0f < hi) || !(l1 - 1.0f >= 1.0f)) break;
                const float ny = tsdf_trilinear(v, l0, l1 + 1.0f, l2) - tsdf_trilinear(v, l0, l1 - 1.0f, l2);
                if (!(l2 + 1.0f < hi) || !(l2 - 1.0f >= 1.0f)) break;
                const float nz = tsdf_trilinear(v, l0, l1, l2 + 1.0f) - tsdf_trilinear(v, l0, l1, l2 - 1.0f);
                const float nn = sqrtf((nx * nx + ny * ny) + nz * nz);
                if (nn == 0.0f) break;
                N[0] = nx / nn;
                N[1] = ny / nn;
                N[2] = nz / nn;
                P[0] = v0 + v.origin[0];
                P[1] = v1 + v.origin[1];
                P[2] = v2 + v.origin[2];
                const int64_t ci = ((int64_t)(int)l0 * res + (int)l1) * res + (int)l2;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float c = 0.0f;
                    if (v.p.color_type == kTsdfRGB8) c = (float)((double)v.p.color[k * v.p.stride + ci] / 255.0);
                    else if (v.p.color_type == kTsdfGray32) c = v.p.color[k * v.p.stride + ci];
                    C[k] = c;
                }
                break;
            }
        }
    } while (false);
}

// block = 16 x 16 pixels, each wave an 8 x 8 tile of it; the blocks of the levels one after the other (level 0 first,
// each level's tiles row by row), a block finds its level from its index.  The levels' pixels are written one level
// after the other, each in pixel order.
static __global__ __launch_bounds__(256) void tsdf_raycast(TsdfVol v, TsdfRaycast a, float* __restrict__ oxyz,
                                                          float* __restrict__ onrm, float* __restrict__ ocol) {
    const int tile = (int)blockIdx.x;
    int lv = 0;
    for (int i = 1; i < a.levels; ++i) lv = tile >= a.level[i].first_tile ? i : lv;
    const TsdfRayLevel& L = a.level[lv];
    const int t = tile - L.first_tile, ty = t / L.tiles_x, tx = t - ty * L.tiles_x;
    const int lane = (int)(threadIdx.x & 63u), wid = (int)(threadIdx.x >> 6);
    const int x = tx * 16 + (wid & 1) * 8 + (lane & 7);
    const int y = ty * 16 + (wid >> 1) * 8 + (lane >> 3);
    if (x >= L.width || y >= L.height) return;
    const int64_t pix = L.first_pixel + (int64_t)y * L.width + x;
    float P[3] = {NAN, NAN, NAN}, N[3] = {NAN, NAN, NAN}, C[3] = {NAN, NAN, NAN};
    tsdf_raycast_pixel(v, a, L, x, y, P, N, C);
    tsdf_store3(oxyz, pix, P[0], P[1], P[2]);
    tsdf_store3(onrm, pix, N[0], N[1], N[2]);
    tsdf_store3(ocol, pix, C[0], C[1], C[2]);
}

// after the scan of the concatenated pixels' flags: end[i] = the kept pixels of the levels 0..i (pos at the next level's
// first pixel; *total where no pixel follows)
static __global__ __launch_bounds__(64) void tsdf_level_ends(TsdfRaycast a, int64_t npix, const uint32_t* __restrict__ pos,
                                                            const uint32_t* __restrict__ total, uint32_t* __restrict__ end) {
    const int i = (int)threadIdx.x;
    if (i >= a.levels) return;
    const int64_t next = i + 1 < a.levels ? a.level[i + 1].first_pixel : npix;
    end[i] = next < npix ? pos[next] : *total;
}

}  // namespace mi
