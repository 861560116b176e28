// occupancy_kernels.h -- geometry::OccupancyGrid (geometry/occupancygrid.cu, densegrid.inl; the cloud of
// geometry/pointcloud_factory.cu:418-430): Insert, AddVoxels, SetFreeArea, the queries and the three extractions.
// include/mi_icp.h holds the numeric contract (operation order); everything below is fp32 with unfused products.
//
// The grid is ONE plane of resolution^3 log-odds (NaN: unknown), indexed (x*res + y)*res + z, z fastest, beside a
// MARK plane of one byte per voxel that is all zero between calls.  The reference keeps 24-byte voxels and, per Insert,
// materialises, filters, sorts, uniques and set-differences n * 3(n_div+1) 12-byte keys.
//   occ_prepare / occ_plan   max |q - viewpoint| over the points: per wave, per block into a partial, one block sums the
//                     partials up and leaves n_div, n_buf and the refusal (n_div above the cap) in the grid's state words
//   occ_mark_rays     one lane per ray walks the reference's VoxelTraversal and stores kOccFree into the mark of every
//                     in-grid voxel it emits.  Every writer of a byte in one launch stores the same value: no atomics,
//                     and the outcome does not depend on arrival order.
//   occ_mark_hits     the next launch stores kOccHit over the marks of the hit points' voxels (free \ occupied is then
//                     "mark == kOccFree" by stream order)
//   occ_mark_indices  AddVoxels: the listed voxels' marks (occ_check_indices has refused a list with an outside index)
//   occ_sweep         16 marks per lane (one 16-byte load); every non-zero one updates its log-odds once and is cleared.
//                     A workgroup whose 4096 marks lie in x-slabs nothing was marked in leaves after reading the slabs'
//                     flags.
//   occ_bounds        the bounds: the marking kernels flag, per axis, every coordinate they marked at (3 * res bytes).
//                     The bounding box of the updated voxels is, per axis, the first and last flagged coordinate --
//                     it cannot be taken from the rays' end voxels, whose walk leaves their box by a voxel.
//   occ_free_box      SetFreeArea          occ_query    the batched point query
//   occ_box_flags / occ_box_gather         the extractions over the bounds box, ascending linear index
// No kernel here keeps an array that is indexed at run time: none uses scratch memory.
#pragma once
#include "device_utils.h"
#include "grid_rules.h"

namespace mi {

constexpr uint8_t kOccFree = 1, kOccHit = 2;
constexpr int kOccSweepBytes = 4096;  // marks per workgroup of occ_sweep; the mark plane is padded to a multiple
// the grid's state words on the device
constexpr int kOccMin = 0, kOccMax = 3, kOccNDiv = 6, kOccNBuf = 7, kOccBad = 8, kOccStateWords = 16;
constexpr int kOccBadNDiv = 1, kOccBadIndex = 2;

struct OccGrid {
    float* prob;     // res^3 log-odds
    uint8_t* marks;  // res^3 bytes, padded with bytes that stay zero
    uint8_t* touch;  // [3][res]: per axis, the coordinates a mark was stored at; zero between calls
    int* state;      // kOccStateWords
    int64_t n;       // res^3
    int res, h_res;
};

struct OccRays {  // Insert's viewpoint and range
    float vp[3];
    float max_range;
};

// every voxel unknown, the bounds back to (h, h, h)
static __global__ __launch_bounds__(256) void occ_reset(OccGrid g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 6) g.state[i] = g.h_res;
    if (i >= g.n) return;
    g.prob[i] = __builtin_nanf("");
}

// The ranged point q of point i (Insert step 1).  0: the point is skipped (a coordinate is not finite), 1: a hit,
// 2: cut at max_range.
__device__ __forceinline__ int occ_ranged_point(const float* __restrict__ pts, int64_t i, const OccRays& a, float* qx,
                                                float* qy, float* qz) {
    const float px = pts[i * 3], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return 0;
    const float dx = px - a.vp[0], dy = py - a.vp[1], dz = pz - a.vp[2];
    const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (a.max_range < 0.0f || dist <= a.max_range) {
        *qx = px;
        *qy = py;
        *qz = pz;
        return 1;
    }
    if (dist == 0.0f) {
        *qx = a.vp[0];
        *qy = a.vp[1];
        *qz = a.vp[2];
    } else {
        *qx = a.vp[0] + (dx / dist) * a.max_range;
        *qy = a.vp[1] + (dy / dist) * a.max_range;
        *qz = a.vp[2] + (dz / dist) * a.max_range;
    }
    return 2;
}

// the maximum of r over the workgroup's four waves
__device__ __forceinline__ uint32_t occ_block_max(uint32_t r) {
    __shared__ uint32_t wmax[4];
    r = wave_max(r);
    if (lane_id() == 0) wmax[threadIdx.x >> 6] = r;
    __syncthreads();
    return max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}

// part[block] = the bits of max_k |q_k - viewpoint_k| over the block's points.  The values are not negative, so their
// bits order as they do, and a NaN (sign cleared) lies above them all: it reaches occ_plan, which refuses.
static __global__ __launch_bounds__(256) void occ_prepare(const float* __restrict__ pts, int64_t n, OccRays a,
                                                         uint32_t* __restrict__ part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t r = 0;
    float qx, qy, qz;
    if (i < n && occ_ranged_point(pts, i, a, &qx, &qy, &qz)) {
        r = max(max(__float_as_uint(fabsf(qx - a.vp[0])), __float_as_uint(fabsf(qy - a.vp[1]))),
                __float_as_uint(fabsf(qz - a.vp[2])));
    }
    r = occ_block_max(r);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// one workgroup: n_div = (int)ceil(max r / voxel_size), n_buf = 3 (n_div + 1); a count above max_ndiv (or no number)
// refuses the call: the marking kernels then do nothing
static __global__ __launch_bounds__(256) void occ_plan(OccGrid g, const uint32_t* __restrict__ part, int64_t nparts, float vs,
                                                      int max_ndiv) {
    uint32_t r = 0;
    for (int64_t i = threadIdx.x; i < nparts; i += 256) r = max(r, part[i]);
    r = occ_block_max(r);
    if (threadIdx.x != 0) return;
    const float max_r = __uint_as_float(r);
    const float nd = ceilf(max_r / vs);
    const bool ok = nd <= (float)max_ndiv;  // (false for a NaN)
    g.state[kOccNDiv] = ok ? (int)nd : 0;
    g.state[kOccNBuf] = ok ? 3 * ((int)nd + 1) : 0;
    g.state[kOccBad] = ok ? 0 : kOccBadNDiv;
}

// has a walk at coordinate c (grid index, before + h), stepping by `step`, left the grid on this axis for good?
__device__ __forceinline__ bool occ_gone(int c, int step, const OccGrid& g) {
    const int i = c + g.h_res;
    return (i < 0 && step <= 0) || (i >= g.res && step >= 0);
}

// the mark of voxel (x, y, z) + h, if that is inside the grid; *in: was it?
__device__ __forceinline__ void occ_mark_at(const OccGrid& g, int x, int y, int z, uint8_t value, bool all_axes, int axis,
                                            bool* in) {
    const int ix = x + g.h_res, iy = y + g.h_res, iz = z + g.h_res;
    *in = cube_inside(g.res, ix, iy, iz);
    if (!*in) return;
    g.marks[cube_index(g.res, ix, iy, iz)] = value;
    if (all_axes || axis == 0) g.touch[ix] = 1;
    if (all_axes || axis == 1) g.touch[g.res + iy] = 1;
    if (all_axes || axis == 2) g.touch[2 * g.res + iz] = 1;
}

// VoxelTraversal(start = viewpoint - origin, end = q - origin) of occupancygrid.cu:60-133, one lane per ray.  The first
// boundary lies HALF a voxel from the start voxel's corner (in double, rounded once), the end voxel is never emitted,
// and at most n_buf voxels are.  A walk that has left the grid on an axis it does not step back along can only emit
// voxels outside the grid: it stops.  One that starts outside walks on exactly, its state must be the reference's
// when it enters.
static __global__ __launch_bounds__(256) void occ_mark_rays(OccGrid g, GridFrame f, const float* __restrict__ pts, int64_t n,
                                                           OccRays a) {
    const int n_buf = g.state[kOccNBuf];
    if (g.state[kOccBad] || g.state[kOccNDiv] <= 0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float qx, qy, qz;
    if (i >= n || !occ_ranged_point(pts, i, a, &qx, &qy, &qz)) return;
    const float vs = f.vs;
    const float sx = a.vp[0] - f.origin[0], sy = a.vp[1] - f.origin[1], sz = a.vp[2] - f.origin[2];
    const float ex = qx - f.origin[0], ey = qy - f.origin[1], ez = qz - f.origin[2];
    float rx = ex - sx, ry = ey - sy, rz = ez - sz;
    const float length = sqrtf((rx * rx + ry * ry) + rz * rz);
    if (length == 0.0f) return;
    rx = rx / length;
    ry = ry / length;
    rz = rz / length;
    int cx = floor_int(sx / vs), cy = floor_int(sy / vs), cz = floor_int(sz / vs);
    const int lx = floor_int(ex / vs), ly = floor_int(ey / vs), lz = floor_int(ez / vs);
    const int stx = rx > 0.0f ? 1 : (rx < 0.0f ? -1 : 0);
    const int sty = ry > 0.0f ? 1 : (ry < 0.0f ? -1 : 0);
    const int stz = rz > 0.0f ? 1 : (rz < 0.0f ? -1 : 0);
    if (occ_gone(cx, stx, g) || occ_gone(cy, sty, g) || occ_gone(cz, stz, g)) return;
    const float bx = (float)(((double)cx + 0.5 * (double)stx) * (double)vs);
    const float by = (float)(((double)cy + 0.5 * (double)sty) * (double)vs);
    const float bz = (float)(((double)cz + 0.5 * (double)stz) * (double)vs);
    float tmx = stx != 0 ? (bx - sx) / rx : INFINITY;
    float tmy = sty != 0 ? (by - sy) / ry : INFINITY;
    float tmz = stz != 0 ? (bz - sz) / rz : INFINITY;
    const float tdx = stx != 0 ? vs / fabsf(rx) : INFINITY;
    const float tdy = sty != 0 ? vs / fabsf(ry) : INFINITY;
    const float tdz = stz != 0 ? vs / fabsf(rz) : INFINITY;

    bool in;
    occ_mark_at(g, cx, cy, cz, kOccFree, true, 0, &in);
    for (int emitted = 1; emitted < n_buf; ++emitted) {
        int axis;
        if (tmx < tmy) axis = tmx < tmz ? 0 : 2;
        else axis = tmy < tmz ? 1 : 2;
        bool gone;
        if (axis == 0) {
            cx += stx;
            tmx += tdx;
            gone = occ_gone(cx, stx, g);
        } else if (axis == 1) {
            cy += sty;
            tmy += tdy;
            gone = occ_gone(cy, sty, g);
        } else {
            cz += stz;
            tmz += tdz;
            gone = occ_gone(cz, stz, g);
        }
        if (cx == lx && cy == ly && cz == lz) break;
        float tmin = tmx < tmy ? tmx : tmy;
        tmin = tmin < tmz ? tmin : tmz;
        if (tmin > length) break;
        if (gone) break;
        const bool was_in = in;
        occ_mark_at(g, cx, cy, cz, kOccFree, !was_in, axis, &in);
    }
}

// the voxels of the hit points: floor((q - origin) / vs) + h
static __global__ __launch_bounds__(256) void occ_mark_hits(OccGrid g, GridFrame f, const float* __restrict__ pts, int64_t n,
                                                           OccRays a) {
    if (g.state[kOccBad]) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float qx, qy, qz;
    if (i >= n || occ_ranged_point(pts, i, a, &qx, &qy, &qz) != 1) return;
    bool in;
    occ_mark_at(g, cell_of(f, qx, 0), cell_of(f, qy, 1), cell_of(f, qz, 2), kOccHit, true, 0, &in);
}

// AddVoxels: an index outside the grid refuses the whole list
static __global__ __launch_bounds__(256) void occ_check_indices(OccGrid g, const int32_t* __restrict__ idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!cube_inside(g.res, idx[i * 3], idx[i * 3 + 1], idx[i * 3 + 2])) g.state[kOccBad] = kOccBadIndex;
}

static __global__ __launch_bounds__(256) void occ_mark_indices(OccGrid g, const int32_t* __restrict__ idx, int64_t n,
                                                              uint8_t value) {
    if (g.state[kOccBad]) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool in;
    occ_mark_at(g, idx[i * 3] - g.h_res, idx[i * 3 + 1] - g.h_res, idx[i * 3 + 2] - g.h_res, value, true, 0, &in);
}

// the update of one voxel: unknown counts as 0, add, clamp (as std::min(std::max(p, lo), hi) selects)
__device__ __forceinline__ float occ_update(float p, float add, float lo, float hi) {
    p = isnan(p) ? 0.0f : p;
    p = p + add;
    p = p < lo ? lo : p;
    return p > hi ? hi : p;
}

__device__ __forceinline__ void occ_sweep_word(const OccGrid& g, uint32_t w, int64_t at, float miss, float hit, float lo,
                                               float hi) {
    if (!w) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t m = (w >> (8 * j)) & 0xffu;
        if (m) g.prob[at + j] = occ_update(g.prob[at + j], m == kOccHit ? hit : miss, lo, hi);
    }
}

// grid: padded mark bytes / 4096.  A non-zero mark is below g.n: the padding stays zero.
static __global__ __launch_bounds__(256) void occ_sweep(OccGrid g, float miss, float hit, float lo, float hi) {
    const int64_t base = (int64_t)blockIdx.x * kOccSweepBytes;
    const int64_t res2 = (int64_t)g.res * g.res;
    const int x_lo = (int)(base / res2), x_hi = (int)min((base + kOccSweepBytes - 1) / res2, (int64_t)g.res - 1);
    bool any = false;
    for (int x = x_lo; x <= x_hi; ++x) any = any || g.touch[x] != 0;
    if (!any) return;
    const int64_t at = base + (int64_t)threadIdx.x * 16;
    uint4* mp = (uint4*)(g.marks + at);
    const uint4 m = *mp;
    if (!(m.x | m.y | m.z | m.w)) return;
    occ_sweep_word(g, m.x, at, miss, hit, lo, hi);
    occ_sweep_word(g, m.y, at + 4, miss, hit, lo, hi);
    occ_sweep_word(g, m.z, at + 8, miss, hit, lo, hi);
    occ_sweep_word(g, m.w, at + 12, miss, hit, lo, hi);
    *mp = make_uint4(0u, 0u, 0u, 0u);
}

// one workgroup, after the sweep: widen the bounds to the flagged coordinates and clear the flags
static __global__ __launch_bounds__(256) void occ_bounds(OccGrid g) {
    __shared__ int lo[3], hi[3];
    if (threadIdx.x < 3) {
        lo[threadIdx.x] = 0x7fffffff;
        hi[threadIdx.x] = -1;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < 3 * g.res; i += 256) {
        if (!g.touch[i]) continue;
        g.touch[i] = 0;
        atomicMin(&lo[i / g.res], i % g.res);
        atomicMax(&hi[i / g.res], i % g.res);
    }
    __syncthreads();
    if (threadIdx.x < 3 && hi[threadIdx.x] >= 0) {
        g.state[kOccMin + threadIdx.x] = min(g.state[kOccMin + threadIdx.x], lo[threadIdx.x]);
        g.state[kOccMax + threadIdx.x] = max(g.state[kOccMax + threadIdx.x], hi[threadIdx.x]);
    }
}

// SetFreeArea: the bounds are OVERWRITTEN with (lo, hi) and every voxel of the box gets the miss, unclamped
static __global__ __launch_bounds__(256) void occ_free_box(OccGrid g, GridBox b, int lo0, int lo1, int lo2, int hi0, int hi1,
                                                          int hi2, float miss) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) {
        g.state[kOccMin] = lo0;
        g.state[kOccMin + 1] = lo1;
        g.state[kOccMin + 2] = lo2;
        g.state[kOccMax] = hi0;
        g.state[kOccMax + 1] = hi1;
        g.state[kOccMax + 2] = hi2;
    }
    if (t >= b.count) return;
    int x, y, z;
    box_voxel(b, t, &x, &y, &z);
    const int64_t i = cube_index(g.res, x, y, z);
    float p = g.prob[i];
    p = isnan(p) ? 0.0f : p;
    g.prob[i] = p + miss;
}

// the voxel of a point, floor((p - origin) / vs) + h per axis, and its log-odds; NaN outside the grid on any axis
static __global__ __launch_bounds__(256) void occ_query(OccGrid g, GridFrame f, const float* __restrict__ pts, int64_t n,
                                                       float* __restrict__ oprob, int32_t* __restrict__ oidx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = cell_of(f, pts[i * 3], 0) + g.h_res;
    const int y = cell_of(f, pts[i * 3 + 1], 1) + g.h_res;
    const int z = cell_of(f, pts[i * 3 + 2], 2) + g.h_res;
    oprob[i] = cube_inside(g.res, x, y, z) ? g.prob[cube_index(g.res, x, y, z)] : __builtin_nanf("");
    if (oidx) {
        oidx[i * 3] = x;
        oidx[i * 3 + 1] = y;
        oidx[i * 3 + 2] = z;
    }
}

// which: 0 known, 1 free (known && p <= thres), 2 occupied (known && p > thres)
static __global__ __launch_bounds__(256) void occ_box_flags(OccGrid g, GridBox b, int which, float thres,
                                                           uint32_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b.count) return;
    int x, y, z;
    box_voxel(b, t, &x, &y, &z);
    const float p = g.prob[cube_index(g.res, x, y, z)];
    const bool known = !isnan(p);
    flags[t] = (known && (which == 0 || (which == 1 ? p <= thres : occupied(p, thres)))) ? 1u : 0u;
}

// the flagged voxels: index, log-odds and (CreateFromOccupancyGrid) the point (index + (0.5 - h)) * vs + origin
static __global__ __launch_bounds__(256) void occ_box_gather(OccGrid g, GridBox b, GridFrame f, const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ pos, int32_t* __restrict__ oidx,
                                                            float* __restrict__ oprob, float* __restrict__ oxyz) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b.count || !flags[t]) return;
    int x, y, z;
    box_voxel(b, t, &x, &y, &z);
    const int64_t p = pos[t];
    if (oidx) {
        oidx[p * 3] = x;
        oidx[p * 3 + 1] = y;
        oidx[p * 3 + 2] = z;
    }
    if (oprob) oprob[p] = g.prob[cube_index(g.res, x, y, z)];
    if (oxyz) {
        const float c = (float)(0.5 - (double)g.h_res);
        oxyz[p * 3] = ((float)x + c) * f.vs + f.origin[0];
        oxyz[p * 3 + 1] = ((float)y + c) * f.vs + f.origin[1];
        oxyz[p * 3 + 2] = ((float)z + c) * f.vs + f.origin[2];
    }
}

}  // namespace mi
