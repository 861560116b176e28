// scalable_tsdf_kernels.h -- integration::ScalableTSDFVolume (integration/scalable_tsdfvolume.{h,cu},
// integrate_functor.h:84-139): a sparse volume of 16^3-voxel units opened around the observed surface.
// include/mi_icp.h holds the numeric contract (operation order); everything below is fp32 with unfused products.
//
// Storage: a pool of unit slots, as planes -- tsdf, weight and (only with a colour type) three colour planes; slot s
// holds [s*4096, (s+1)*4096) of each plane, a voxel at x*256 + y*16 + z inside it.
// Directory: the open units' packed keys in ascending order, each with its slot.  A key packs the three unit indices,
// biased by 2^20, into 21 bits each (x highest): ascending packed keys are ascending (x, y, z).  A lookup is a binary
// search of that list (DESIGN says why not a hash table).
//   stsdf_open<false / true>   per sampled depth pixel: its world point (depth_kernels.h back_project, so bit-equal to
//                     CreateFromDepthImage), the units within sdf_trunc of it, and of those the ones the directory does
//                     not hold -- counted, then after the scan written as sort keys
//   (radix_sort_pairs) + stsdf_heads + (scan) + stsdf_new_keys   the frame's new keys once each, ascending
//   stsdf_merge       old and new lists into the other directory buffer: every entry's place is its own rank plus the
//                     number of entries of the other list below it.  New key j gets slot n_old + j.
//   (tsdf_reset)      the new slots' voxels
//   stsdf_integrate   one workgroup per open unit, a wave on four 16-z columns; every voxel goes through
//                     tsdf_update_voxel (tsdf_kernels.h), the one per-voxel rule of both volumes
//   stsdf_voxel_flags / stsdf_voxel_gather   ExtractVoxelPointCloud, over the directory's order
//   stsdf_cloud_count / stsdf_cloud_list / stsdf_cloud_points   ExtractPointCloud: per voxel the number of crossing
//                     edges; after the scan the edges as a compact list; then one lane per surface point
//   stsdf_gather_units   the read-back
// The planes (TsdfPlanes), their reset, the rule and the emit paths' colour blend, normalisation and grey are those of
// tsdf_kernels.h, which also says what the two volumes keep apart.
// No kernel here keeps an array that is indexed at run time: none uses scratch memory.
#pragma once
#include "depth_kernels.h"
#include "tsdf_kernels.h"

namespace mi {

constexpr int kStsdfRes = 16, kStsdfUnit = 4096;
constexpr int kStsdfKeyMax = (1 << 20) - 1;  // a unit index lies within +-kStsdfKeyMax

__host__ __device__ __forceinline__ bool stsdf_key_ok(int x, int y, int z) {
    return x >= -kStsdfKeyMax && x <= kStsdfKeyMax && y >= -kStsdfKeyMax && y <= kStsdfKeyMax && z >= -kStsdfKeyMax &&
           z <= kStsdfKeyMax;
}

__host__ __device__ __forceinline__ uint64_t stsdf_pack(int x, int y, int z) {
    return ((uint64_t)(uint32_t)(x + (1 << 20)) << 42) | ((uint64_t)(uint32_t)(y + (1 << 20)) << 21) |
           (uint64_t)(uint32_t)(z + (1 << 20));
}

__host__ __device__ __forceinline__ void stsdf_unpack(uint64_t k, int* x, int* y, int* z) {
    *x = (int)((k >> 42) & 0x1fffffu) - (1 << 20);
    *y = (int)((k >> 21) & 0x1fffffu) - (1 << 20);
    *z = (int)(k & 0x1fffffu) - (1 << 20);
}

struct StsdfDir {
    const uint64_t* keys;   // [n] ascending
    const uint32_t* slots;  // [n]
    int n;
};

// number of keys below `key`
__device__ __forceinline__ int stsdf_lower(const uint64_t* __restrict__ keys, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the slot of unit (x, y, z), or -1 when it is not open (or cannot be)
__device__ __forceinline__ int stsdf_find(const StsdfDir& d, int x, int y, int z) {
    if (!stsdf_key_ok(x, y, z)) return -1;
    const uint64_t key = stsdf_pack(x, y, z);
    const int i = stsdf_lower(d.keys, d.n, key);
    return (i < d.n && d.keys[i] == key) ? (int)d.slots[i] : -1;
}

struct StsdfVol {
    TsdfPlanes p;  // stride = capacity * 4096
    float voxel_length, half, unit_length;  // half = 0.5 * voxel_length, unit_length = voxel_length * 16.0f
    float sdf_trunc;
};

// ---- open -----------------------------------------------------------------------------------------------------------
// WRITE = false: cnt[idx] = number of units pixel idx wants that are not open.  WRITE = true: their keys at pos[idx]...
template <bool WRITE>
static __global__ __launch_bounds__(256) void stsdf_open(DepthArgs a, int64_t count, float trunc, float L, StsdfDir dir,
                                                        uint32_t* __restrict__ cnt, const uint32_t* __restrict__ pos,
                                                        uint64_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    int row, col;
    strided_pixel(a, idx, row, col);
    float p[3];
    back_project(a, row, col, p);
    uint32_t n = 0;
    if (finite3(p)) {
        int lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = floor_int((p[k] - trunc) / L);
            hi[k] = min(floor_int((p[k] + trunc) / L), lo[k] + 3);  // (sdf_trunc <= L: never more than three apart)
        }
        const uint32_t base = WRITE ? pos[idx] : 0u;
        for (int x = lo[0]; x <= hi[0]; ++x)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int z = lo[2]; z <= hi[2]; ++z) {
                    if (!stsdf_key_ok(x, y, z) || stsdf_find(dir, x, y, z) >= 0) continue;
                    if (WRITE) {
                        keys_out[base + n] = stsdf_pack(x, y, z);
                        vals_out[base + n] = base + n;
                    }
                    ++n;
                }
    }
    if (!WRITE) cnt[idx] = n;
}

// sorted candidates: 1 where a key differs from the one before it
static __global__ __launch_bounds__(256) void stsdf_heads(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

static __global__ __launch_bounds__(256) void stsdf_new_keys(const uint64_t* __restrict__ keys, int64_t n,
                                                            const uint32_t* __restrict__ pos, uint64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || keys[i] != keys[i - 1]) out[pos[i]] = keys[i];
}

// old[n_old] (with slots) and fresh[n_new] (slot n_old + j), both ascending and disjoint, into one ascending list
static __global__ __launch_bounds__(256) void stsdf_merge(StsdfDir old, const uint64_t* __restrict__ fresh, int n_new,
                                                         uint64_t* __restrict__ keys_out, uint32_t* __restrict__ slots_out) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < old.n) {
        const uint64_t k = old.keys[i];
        const int at = i + stsdf_lower(fresh, n_new, k);
        keys_out[at] = k;
        slots_out[at] = old.slots[i];
    } else if (i < old.n + n_new) {
        const int j = i - old.n;
        const uint64_t k = fresh[j];
        const int at = j + stsdf_lower(old.keys, old.n, k);
        keys_out[at] = k;
        slots_out[at] = (uint32_t)i;
    }
}

// ---- integrate ------------------------------------------------------------------------------------------------------
// block = one open unit (directory entry blockIdx.x); thread t takes voxels (x, t >> 4, t & 15), x = 0..15: a wave reads
// and writes four whole 16-z columns, 256 consecutive bytes of a plane, per step.
static __global__ __launch_bounds__(256) void stsdf_integrate(StsdfVol v, StsdfDir dir, TsdfIntegrate a) {
    const int e = (int)blockIdx.x;
    if (e >= dir.n) return;
    int kx, ky, kz;
    stsdf_unpack(dir.keys[e], &kx, &ky, &kz);
    const int64_t base = (int64_t)dir.slots[e] * kStsdfUnit;
    const float ox = (float)kx * v.unit_length, oy = (float)ky * v.unit_length, oz = (float)kz * v.unit_length;
    const int y = (int)(threadIdx.x >> 4), z = (int)(threadIdx.x & 15u);
    const float py = (v.half + v.voxel_length * (float)y) + oy;
    const float pz = v.half + oz;
    const float zf = (float)z;
    for (int x = 0; x < kStsdfRes; ++x) {
        const float px = (v.half + v.voxel_length * (float)x) + ox;
        const float X = (((a.E[0][0] * px + a.E[0][1] * py) + a.E[0][2] * pz) + a.E[0][3]) + zf * a.D[0];
        const float Y = (((a.E[1][0] * px + a.E[1][1] * py) + a.E[1][2] * pz) + a.E[1][3]) + zf * a.D[1];
        const float Z = (((a.E[2][0] * px + a.E[2][1] * py) + a.E[2][2] * pz) + a.E[2][3]) + zf * a.D[2];
        tsdf_update_voxel(v.p, base + x * 256 + (int)threadIdx.x, X, Y, Z, a);
    }
}

// ---- extraction -----------------------------------------------------------------------------------------------------
// candidate j = directory entry j / 4096, voxel j % 4096

static __global__ __launch_bounds__(256) void stsdf_voxel_flags(StsdfVol v, StsdfDir dir, int64_t n, uint32_t* __restrict__ flags) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t i = (int64_t)dir.slots[j >> 12] * kStsdfUnit + (j & 4095);
    flags[j] = tsdf_valid(v.p.weight[i], v.p.tsdf[i]) ? 1u : 0u;
}

static __global__ __launch_bounds__(256) void stsdf_voxel_gather(StsdfVol v, StsdfDir dir, int64_t n,
                                                                const uint32_t* __restrict__ flags,
                                                                const uint32_t* __restrict__ pos, float* __restrict__ oxyz,
                                                                float* __restrict__ ocol) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !flags[j]) return;
    const int e = (int)(j >> 12), vox = (int)(j & 4095);
    const int64_t i = (int64_t)dir.slots[e] * kStsdfUnit + vox;
    int key[3];
    stsdf_unpack(dir.keys[e], &key[0], &key[1], &key[2]);
    const int xyz[3] = {vox >> 8, (vox >> 4) & 15, vox & 15};
    const int64_t p = pos[j];
#pragma unroll
    for (int k = 0; k < 3; ++k) oxyz[p * 3 + k] = (v.half + v.voxel_length * (float)xyz[k]) + (float)key[k] * v.unit_length;
    const float c = tsdf_grey(v.p.tsdf[i]);
    ocol[p * 3] = c;
    ocol[p * 3 + 1] = c;
    ocol[p * 3 + 2] = c;
}

// voxel 1 of the edge from voxel (x, y, z) of the unit `key` in slot `slot` along AX: its plane index, or -1 when it
// lies in a unit that is not open
template <int AX>
__device__ __forceinline__ int64_t stsdf_next(const StsdfDir& dir, const int key[3], int slot, int vox) {
    const int c = AX == 0 ? vox >> 8 : (AX == 1 ? (vox >> 4) & 15 : vox & 15);
    const int step = AX == 0 ? 256 : (AX == 1 ? 16 : 1);
    if (c + 1 < kStsdfRes) return (int64_t)slot * kStsdfUnit + vox + step;
    const int s1 = stsdf_find(dir, key[0] + (AX == 0), key[1] + (AX == 1), key[2] + (AX == 2));
    return s1 < 0 ? -1 : (int64_t)s1 * kStsdfUnit + (vox - 15 * step);
}

template <int AX>
__device__ __forceinline__ bool stsdf_edge(const StsdfVol& v, const StsdfDir& dir, const int key[3], int slot, int vox, float f0,
                                           int64_t* i1, float* f1) {
    *i1 = stsdf_next<AX>(dir, key, slot, vox);
    if (*i1 < 0) return false;  // (weight 0)
    *f1 = v.p.tsdf[*i1];
    return tsdf_valid(v.p.weight[*i1], *f1) && f0 * *f1 < 0.0f;
}

static __global__ __launch_bounds__(256) void stsdf_cloud_count(StsdfVol v, StsdfDir dir, int64_t n, uint32_t* __restrict__ count) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int e = (int)(j >> 12), vox = (int)(j & 4095);
    const int slot = (int)dir.slots[e];
    const int64_t i0 = (int64_t)slot * kStsdfUnit + vox;
    const float f0 = v.p.tsdf[i0];
    uint32_t cnt = 0;
    if (tsdf_valid(v.p.weight[i0], f0)) {
        int key[3];
        stsdf_unpack(dir.keys[e], &key[0], &key[1], &key[2]);
        int64_t i1;
        float f1;
        cnt += stsdf_edge<0>(v, dir, key, slot, vox, f0, &i1, &f1) ? 1u : 0u;
        cnt += stsdf_edge<1>(v, dir, key, slot, vox, f0, &i1, &f1) ? 1u : 0u;
        cnt += stsdf_edge<2>(v, dir, key, slot, vox, f0, &i1, &f1) ? 1u : 0u;
    }
    count[j] = cnt;
}

// GetTSDFAt at the world point p: 0 where the unit of (p - half) is not open; a corner in a unit that is not open
// counts as 0
__device__ __forceinline__ float stsdf_at(const StsdfVol& v, const StsdfDir& dir, float p0, float p1, float p2) {
    const float pl[3] = {p0 - v.half, p1 - v.half, p2 - v.half};
    int u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = floor_int(pl[k] / v.unit_length);
    const int s0 = stsdf_find(dir, u[0], u[1], u[2]);
    if (s0 < 0) return 0.0f;
    int i[3];
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float g = (pl[k] - (float)u[k] * v.unit_length) / v.voxel_length;
        i[k] = min(max(floor_int(g), 0), kStsdfRes - 1);
        r[k] = g - (float)i[k];
    }
    // the corners (dx, dy, dz); a coordinate of 16 is coordinate 0 of the next unit along that axis
    float f[2][2][2];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) {
                const int cx = i[0] + dx, cy = i[1] + dy, cz = i[2] + dz;
                const int wx = cx >= kStsdfRes, wy = cy >= kStsdfRes, wz = cz >= kStsdfRes;
                int s = s0;
                if (wx | wy | wz) s = stsdf_find(dir, u[0] + wx, u[1] + wy, u[2] + wz);
                f[dx][dy][dz] =
                    s < 0 ? 0.0f : v.p.tsdf[(int64_t)s * kStsdfUnit + (cx - 16 * wx) * 256 + (cy - 16 * wy) * 16 + (cz - 16 * wz)];
            }
    const float a0 = 1.0f - r[0], a1 = 1.0f - r[1], a2 = 1.0f - r[2];
    return a0 * (a1 * (a2 * f[0][0][0] + r[2] * f[0][0][1]) + r[1] * (a2 * f[0][1][0] + r[2] * f[0][1][1])) +
           r[0] * (a1 * (a2 * f[1][0][0] + r[2] * f[1][0][1]) + r[1] * (a2 * f[1][1][0] + r[2] * f[1][1][1]));
}

// One surface point: the edge from voxel `vox` of directory entry e (plane index i0, tsdf f0) along `ax` to the voxel
// at plane index i1 (tsdf f1).  The axis is a run-time value chosen by selects, so that the lanes of a wave, each with
// its own axis, stay together through the six trilinear samples of the normal.
__device__ __forceinline__ void stsdf_cloud_emit(const StsdfVol& v, const StsdfDir& dir, const int key[3], int vox, int ax,
                                                 int64_t i0, int64_t i1, float f0, float f1, int64_t p,
                                                 float* __restrict__ oxyz, float* __restrict__ onrm, float* __restrict__ ocol) {
    const float r0 = fabsf(f0), r1 = fabsf(f1), rs = r0 + r1;
    float q0 = (v.half + v.voxel_length * (float)(vox >> 8)) + (float)key[0] * v.unit_length;
    float q1 = (v.half + v.voxel_length * (float)((vox >> 4) & 15)) + (float)key[1] * v.unit_length;
    float q2 = (v.half + v.voxel_length * (float)(vox & 15)) + (float)key[2] * v.unit_length;
    const float qa = ax == 0 ? q0 : (ax == 1 ? q1 : q2);
    const float qn = (qa * r1 + (qa + v.voxel_length) * r0) / rs;
    q0 = ax == 0 ? qn : q0;
    q1 = ax == 1 ? qn : q1;
    q2 = ax == 2 ? qn : q2;
    oxyz[p * 3] = q0;
    oxyz[p * 3 + 1] = q1;
    oxyz[p * 3 + 2] = q2;
    if (ocol) {
#pragma unroll
        for (int k = 0; k < 3; ++k) ocol[p * 3 + k] = tsdf_blend_color(v.p, k, i0, i1, r0, r1, rs);
    }
    // GetNormalAt: half_gap is a float here
    const float gap = (float)(0.99 * (double)v.voxel_length);
    float n[3];
    n[0] = stsdf_at(v, dir, q0 + gap, q1, q2) - stsdf_at(v, dir, q0 - gap, q1, q2);
    n[1] = stsdf_at(v, dir, q0, q1 + gap, q2) - stsdf_at(v, dir, q0, q1 - gap, q2);
    n[2] = stsdf_at(v, dir, q0, q1, q2 + gap) - stsdf_at(v, dir, q0, q1, q2 - gap);
    tsdf_normalize(n);
#pragma unroll
    for (int k = 0; k < 3; ++k) onrm[p * 3 + k] = n[k];
}

// the crossing edges as a list in output order: entry p = candidate * 4 + axis (a candidate is below 2^30)
static __global__ __launch_bounds__(256) void stsdf_cloud_list(StsdfVol v, StsdfDir dir, int64_t n,
                                                              const uint32_t* __restrict__ count,
                                                              const uint32_t* __restrict__ pos, uint32_t* __restrict__ list) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !count[j]) return;
    const int e = (int)(j >> 12), vox = (int)(j & 4095);
    const int slot = (int)dir.slots[e];
    const float f0 = v.p.tsdf[(int64_t)slot * kStsdfUnit + vox];
    int key[3];
    stsdf_unpack(dir.keys[e], &key[0], &key[1], &key[2]);
    int64_t p = pos[j], i1;
    float f1;
    if (stsdf_edge<0>(v, dir, key, slot, vox, f0, &i1, &f1)) list[p++] = (uint32_t)j * 4u;
    if (stsdf_edge<1>(v, dir, key, slot, vox, f0, &i1, &f1)) list[p++] = (uint32_t)j * 4u + 1u;
    if (stsdf_edge<2>(v, dir, key, slot, vox, f0, &i1, &f1)) list[p++] = (uint32_t)j * 4u + 2u;
}

// one lane per surface point: every lane of a wave has work (a lane per voxel left one lane in dozens busy)
static __global__ __launch_bounds__(256) void stsdf_cloud_points(StsdfVol v, StsdfDir dir, int64_t m,
                                                                const uint32_t* __restrict__ list, float* __restrict__ oxyz,
                                                                float* __restrict__ onrm, float* __restrict__ ocol) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= m) return;
    const uint32_t id = list[p];
    const int64_t j = (int64_t)(id >> 2);
    const int ax = (int)(id & 3u);
    const int e = (int)(j >> 12), vox = (int)(j & 4095);
    const int slot = (int)dir.slots[e];
    const int64_t i0 = (int64_t)slot * kStsdfUnit + vox;
    int key[3];
    stsdf_unpack(dir.keys[e], &key[0], &key[1], &key[2]);
    const int64_t i1 = ax == 0 ? stsdf_next<0>(dir, key, slot, vox) : (ax == 1 ? stsdf_next<1>(dir, key, slot, vox) : stsdf_next<2>(dir, key, slot, vox));
    if (i1 < 0) return;  // (the list holds crossing edges only: voxel 1 is there)
    stsdf_cloud_emit(v, dir, key, vox, ax, i0, i1, v.p.tsdf[i0], v.p.tsdf[i1], p, oxyz, onrm, ocol);
}

// ---- read-back ------------------------------------------------------------------------------------------------------
// keys[e][3] and, in the directory's order, every unit's planes: tsdf / weight [n][4096], colour [3][n][4096]
static __global__ __launch_bounds__(256) void stsdf_gather_units(StsdfVol v, StsdfDir dir, int64_t n, int32_t* __restrict__ keys,
                                                                float* __restrict__ tsdf, float* __restrict__ weight,
                                                                float* __restrict__ color) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int e = (int)(j >> 12), vox = (int)(j & 4095);
    const int64_t i = (int64_t)dir.slots[e] * kStsdfUnit + vox;
    if (keys && vox < 3) {
        int key[3];
        stsdf_unpack(dir.keys[e], &key[0], &key[1], &key[2]);
        keys[(int64_t)e * 3 + vox] = vox == 0 ? key[0] : (vox == 1 ? key[1] : key[2]);
    }
    if (tsdf) tsdf[j] = v.p.tsdf[i];
    if (weight) weight[j] = v.p.weight[i];
    if (color) {
#pragma unroll
        for (int k = 0; k < 3; ++k) color[k * n + j] = v.p.color[k * v.p.stride + i];
    }
}

}  // namespace mi
