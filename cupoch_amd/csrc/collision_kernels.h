// collision_kernels.h -- collision::ComputeIntersection and CreateVoxelGrid (collision/{collision,primitives}.cu).
//
// The reference builds an LBVH over the target and walks it per query with a stack buffer of 10,000 hits.  Here the
// side that is searched (ColGrid) is addressed directly: a VoxelGrid's keys ascend, so a cell is a binary search and a
// run of cells of one x a contiguous range; an occupancy grid is its dense log-odds plane.  What is searched is the
// integer box of cells an enumerated element can reach (collision_predicates.h: THE CANDIDATE CELLS):
//   col_cells_grid    a lane per enumerated voxel: the exact range of cells per axis, x-major, first hit
//   col_lines_grid    a wave per line: one x-slab at a time, the line's y / z range inside the slab, lanes stride the
//                     slab's cells (occupancy grid) or its voxels (VoxelGrid), minimum over the wave
//   col_prims_grid    a workgroup per primitive: the same over the primitive's reach, the slabs dealt among four waves
//   col_cells_prims   a lane per enumerated voxel, the primitives in order behind the reject of col_prim_reach
// x-major order visits a sorted VoxelGrid's indices and an occupancy grid's linear indices ascending, so the first slab
// (the first cell) with a hit ends the work; a VoxelGrid that came unsorted is searched through its sorted copy and
// perm[], and then the minimum of perm over all hits is taken.  Every kernel writes hit[i]: the other side's index or -1;
// flags + the scan + col_emit_pairs compact them.  No atomics.  The code object reports 28 bytes of
// scratch per lane for col_prims_grid, col_cells_prims and col_voxelize_flags, and none for every other kernel here.
#pragma once
#include "collision_predicates.h"
#include "device_utils.h"
#include "voxelgrid_kernels.h"

namespace mi {

struct ColGrid {           // the side that is searched
    int occ;               // 0: a VoxelGrid's keys, 1: an occupancy grid's plane
    const int32_t* keys;   // [m][3] ascending, distinct
    const uint32_t* perm;  // sorted position -> the caller's index; null: the keys are the caller's own
    int64_t m;
    const int32_t* ext;    // device words: min[3], max[3] of the keys
    const float* prob;     // res^3 log-odds
    int res, h;
    int b[6];              // the bounds box, inclusive, as grid indices
    float thres;
    GridFrame f;
};

struct ColCells {  // the enumerated voxels: keys[n][3]; res > 0: they are occupancy-grid indices, key = index - h
    const int32_t* keys;
    int64_t n;
    int res, h;
    GridFrame f;
};

constexpr int32_t kColNone = 0x7fffffff;

__device__ __forceinline__ void col_key_span(const ColGrid& G, int a, int32_t* klo, int32_t* khi) {
    if (G.occ) {
        *klo = G.b[a] - G.h;
        *khi = G.b[3 + a] - G.h;
    } else {
        *klo = a == 0 ? max(G.ext[a], kVgNoKey + 1) : G.ext[a];  // (a key whose x is kVgNoKey is no key)
        *khi = G.ext[3 + a];
    }
}

// the smallest x >= x0 that a key of a VoxelGrid has; above every key: none (an occupancy grid has every x)
__device__ __forceinline__ int64_t col_next_x(const ColGrid& G, int64_t x0) {
    if (G.occ) return x0;
    if (x0 > INT32_MAX) return (int64_t)INT32_MAX + 1;
    const int64_t p = keys3_lower(G.keys, G.m, (int32_t)x0, INT32_MIN, INT32_MIN);
    return p < G.m ? (int64_t)G.keys[p * 3] : (int64_t)INT32_MAX + 1;
}

__device__ __forceinline__ bool col_occupied(const ColGrid& G, int64_t idx) { return occupied(G.prob[idx], G.thres); }

__device__ __forceinline__ int32_t col_wave_min_all(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ void col_cell_box(const ColGrid& G, int32_t x, int32_t y, int32_t z, float* lo, float* hi) {
    lo[0] = col::cell_lo(x, G.f.vs, G.f.origin[0]);
    hi[0] = col::cell_hi(x, G.f.vs, G.f.origin[0]);
    lo[1] = col::cell_lo(y, G.f.vs, G.f.origin[1]);
    hi[1] = col::cell_hi(y, G.f.vs, G.f.origin[1]);
    lo[2] = col::cell_lo(z, G.f.vs, G.f.origin[2]);
    hi[2] = col::cell_hi(z, G.f.vs, G.f.origin[2]);
}

// ---- voxels against a grid: the cell-cell predicate is the candidate range itself, so every cell present in it is a hit
static __global__ __launch_bounds__(256) void col_cells_grid(ColCells E, ColGrid G, float margin, int32_t* __restrict__ hit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= E.n) return;
    int32_t r0[3], r1[3];
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        const int32_t k = E.keys[i * 3 + a] - (E.res > 0 ? E.h : 0);
        const float alo = col::cell_lo(k, E.f.vs, E.f.origin[a]) - margin, ahi = col::cell_hi(k, E.f.vs, E.f.origin[a]) + margin;
        int32_t klo, khi;
        col_key_span(G, a, &klo, &khi);
        col::cell_range(alo, ahi, G.f.vs, G.f.origin[a], klo, khi, &r0[a], &r1[a]);
        empty = empty || r0[a] > r1[a];
    }
    int32_t best = kColNone;
    if (!empty && G.occ) {
        for (int32_t x = r0[0]; x <= r1[0] && best == kColNone; ++x)
            for (int32_t y = r0[1]; y <= r1[1] && best == kColNone; ++y) {
                const int64_t row = cube_index(G.res, x + G.h, y + G.h, G.h);
                for (int32_t z = r0[2]; z <= r1[2]; ++z)
                    if (col_occupied(G, row + z)) {
                        best = (int32_t)(row + z);
                        break;
                    }
            }
    } else if (!empty) {
        const int64_t p0 = keys3_lower(G.keys, G.m, r0[0], r0[1], r0[2]);
        const int64_t p1 = keys3_upper(G.keys, G.m, r1[0], r1[1], r1[2]);
        // fewer voxels between the corners than a search per column would cost: walk them.  (cols below 2^28 each
        // before they are multiplied, so no product overflows whatever the key extents)
        const int64_t nx = (int64_t)r1[0] - r0[0] + 1, ny = (int64_t)r1[1] - r0[1] + 1, cols = (p1 - p0 + 7) >> 3;
        if (nx >= cols || ny >= cols || nx * ny >= cols) {
            for (int64_t p = p0; p < p1; ++p) {
                const int32_t y = G.keys[p * 3 + 1], z = G.keys[p * 3 + 2];
                if (y < r0[1] || y > r1[1] || z < r0[2] || z > r1[2]) continue;
                if (!G.perm) {
                    best = (int32_t)p;
                    break;
                }
                best = min(best, (int32_t)G.perm[p]);
            }
        } else {
            for (int32_t x = r0[0]; x <= r1[0]; ++x) {
                for (int32_t y = r0[1]; y <= r1[1]; ++y) {
                    for (int64_t p = keys3_lower(G.keys, G.m, x, y, r0[2]); p < G.m; ++p) {
                        if (G.keys[p * 3] != x || G.keys[p * 3 + 1] != y || G.keys[p * 3 + 2] > r1[2]) break;
                        best = min(best, G.perm ? (int32_t)G.perm[p] : (int32_t)p);
                        if (!G.perm) break;
                    }
                    if (!G.perm && best != kColNone) break;
                }
                if (!G.perm && best != kColNone) break;
            }
        }
    }
    hit[i] = best == kColNone ? -1 : best;
}

// ---- one x-slab of the searched grid, by a wave: the smallest index among the cells (y0..y1, z0..z1) that are there and
// that pred(lo, hi) accepts; every lane gets the wave's minimum
template <class Pred>
__device__ __forceinline__ int32_t col_slab_min(const ColGrid& G, int lane, int32_t x, int32_t y0, int32_t y1, int32_t z0, int32_t z1,
                                                Pred pred) {
    int32_t best = kColNone;
    float lo[3], hi[3];
    if (y0 > y1 || z0 > z1) return best;  // (the same on every lane)
    if (G.occ) {
        const int64_t nz = (int64_t)z1 - z0 + 1, cnt = ((int64_t)y1 - y0 + 1) * nz;
        for (int64_t t = lane; t < cnt; t += 64) {
            const int32_t y = y0 + (int32_t)(t / nz), z = z0 + (int32_t)(t % nz);
            const int64_t idx = cube_index(G.res, x + G.h, y + G.h, z + G.h);
            if (!col_occupied(G, idx)) continue;
            col_cell_box(G, x, y, z, lo, hi);
            if (pred(lo, hi)) {
                best = (int32_t)idx;  // (a lane's cells ascend)
                break;
            }
        }
    } else {
        const int64_t p0 = keys3_lower(G.keys, G.m, x, y0, z0), p1 = keys3_upper(G.keys, G.m, x, y1, z1);
        for (int64_t p = p0 + lane; p < p1; p += 64) {
            const int32_t y = G.keys[p * 3 + 1], z = G.keys[p * 3 + 2];
            if (z < z0 || z > z1) continue;
            col_cell_box(G, x, y, z, lo, hi);
            if (pred(lo, hi)) {
                best = min(best, G.perm ? (int32_t)G.perm[p] : (int32_t)p);
                if (!G.perm) break;
            }
        }
    }
    return col_wave_min_all(best);
}

// the range of keys along axis a whose cells meet [blo, bhi]; false: none
__device__ __forceinline__ bool col_axis_range(const ColGrid& G, int a, float blo, float bhi, int32_t* k0, int32_t* k1) {
    int32_t klo, khi;
    col_key_span(G, a, &klo, &khi);
    if (klo > khi) return false;
    col::cell_range(blo, bhi, G.f.vs, G.f.origin[a], klo, khi, k0, k1);
    return *k0 <= *k1;
}

// ---- lines against a grid: a wave per line
static __global__ __launch_bounds__(256) void col_lines_grid(const float* __restrict__ pts, const int32_t* __restrict__ lines, int64_t nl,
                                                            ColGrid G, float margin, int32_t* __restrict__ hit) {
    const int lane = lane_id();
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= nl) return;
    const int64_t ia = lines[e * 2], ib = lines[e * 2 + 1];
    const float p0[3] = {pts[ia * 3], pts[ia * 3 + 1], pts[ia * 3 + 2]};
    const float p1[3] = {pts[ib * 3], pts[ib * 3 + 1], pts[ib * 3 + 2]};
    int32_t best = kColNone;
    float s[3];
    int32_t klo[3], khi[3], r0[3], r1[3], k0[3], k1[3];
    for (int a = 0; a < 3; ++a) col_key_span(G, a, &klo[a], &khi[a]);
    if (col::segment_cells(p0, p1, margin, G.f.vs, G.f.origin, klo, khi, s, r0, r1)) {
        auto pred = [&](const float* lo, const float* hi) {
            const float ilo[3] = {lo[0] - margin, lo[1] - margin, lo[2] - margin};
            const float ihi[3] = {hi[0] + margin, hi[1] + margin, hi[2] + margin};
            return col::segment_cell(p0, p1, ilo, ihi);
        };
        // slab by slab, over the x a VoxelGrid has keys at: the cost follows the voxels that exist, not the extents
        for (int64_t x = col_next_x(G, r0[0]); x <= r1[0]; x = col_next_x(G, x + 1)) {
            if (!col::segment_slab_cells(p0, p1, margin, s, G.f.vs, G.f.origin, (int32_t)x, r0, r1, k0, k1)) continue;
            best = min(best, col_slab_min(G, lane, (int32_t)x, k0[1], k1[1], k0[2], k1[2], pred));
            if (!G.perm && best != kColNone) break;
        }
    }
    if (lane == 0) hit[e] = best == kColNone ? -1 : best;
}

// ---- primitives against a grid: a workgroup per primitive, the x-slabs dealt among its four waves (few primitives, each
// with up to the whole grid in reach: a wave apiece would leave most of the device idle).  A wave stops at its first slab
// with a hit -- its own slabs ascend -- and the smallest of the four is the primitive's.
static __global__ __launch_bounds__(256) void col_prims_grid(const mi_icp_primitive* __restrict__ prims, int64_t np, ColGrid G, float margin,
                                                            int32_t* __restrict__ hit) {
    __shared__ int32_t found[4];
    const int lane = lane_id(), wid = (int)(threadIdx.x >> 6);
    const int64_t e = blockIdx.x;
    if (e >= np) return;  // (the whole block)
    const mi_icp_primitive P = prims[e];
    int32_t best = kColNone;
    bool live = col::primitive_live(P);
    int32_t r0[3], r1[3];
    if (live) {
        float blo[3], bhi[3];
        col::primitive_reach(P, margin, G.f.vs, blo, bhi);
        for (int a = 0; a < 3 && live; ++a) live = col_axis_range(G, a, blo[a], bhi[a], &r0[a], &r1[a]);
    }
    if (live) {
        auto pred = [&](const float* lo, const float* hi) { return col::primitive_cell(P, lo, hi, margin); };
        // wave wid takes the slabs r0 + wid, + 4, ...; of a VoxelGrid only those it has keys at
        for (int64_t x = (int64_t)r0[0] + wid; x <= r1[0];) {
            const int64_t nx = col_next_x(G, x);
            if (nx != x) {  // (nx > x: the first slab of this wave's at or after it)
                x = nx + ((wid - (nx - r0[0])) & 3);
                continue;
            }
            best = min(best, col_slab_min(G, lane, (int32_t)x, r0[1], r1[1], r0[2], r1[2], pred));
            if (!G.perm && best != kColNone) break;
            x += 4;
        }
    }
    if (lane == 0) found[wid] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        best = min(min(found[0], found[1]), min(found[2], found[3]));
        hit[e] = best == kColNone ? -1 : best;
    }
}

// a primitive's reach against cells of size vs: lo[3], hi[3]; one that cannot collide gets lo = +inf
static __global__ __launch_bounds__(256) void col_prim_reach(const mi_icp_primitive* __restrict__ prims, int64_t np, float margin, float vs,
                                                            float* __restrict__ reach) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    const mi_icp_primitive P = prims[j];
    float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (col::primitive_live(P)) col::primitive_reach(P, margin, vs, blo, bhi);
    for (int k = 0; k < 3; ++k) {
        reach[j * 6 + k] = blo[k];
        reach[j * 6 + 3 + k] = bhi[k];
    }
}

// ---- voxels against primitives: a lane per voxel, the primitives in order, the first that collides
static __global__ __launch_bounds__(256) void col_cells_prims(ColCells E, const mi_icp_primitive* __restrict__ prims,
                                                             const float* __restrict__ reach, int64_t np, float margin,
                                                             int32_t* __restrict__ hit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= E.n) return;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        const int32_t k = E.keys[i * 3 + a] - (E.res > 0 ? E.h : 0);
        lo[a] = col::cell_lo(k, E.f.vs, E.f.origin[a]);
        hi[a] = col::cell_hi(k, E.f.vs, E.f.origin[a]);
    }
    int32_t best = -1;
    for (int64_t j = 0; j < np; ++j) {
        const float* r = reach + j * 6;
        if (!(hi[0] >= r[0] && lo[0] <= r[3] && hi[1] >= r[1] && lo[1] <= r[4] && hi[2] >= r[2] && lo[2] <= r[5])) continue;
        if (col::primitive_cell(prims[j], lo, hi, margin)) {
            best = (int32_t)j;
            break;
        }
    }
    hit[i] = best;
}

// a line's point indices inside [0, npts)?  *status != 0: no
static __global__ __launch_bounds__(256) void col_check_lines(const int32_t* __restrict__ lines, int64_t nl, int64_t npts,
                                                             uint32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nl) return;
    const int32_t a = lines[i * 2], b = lines[i * 2 + 1];
    if (a < 0 || a >= npts || b < 0 || b >= npts) *status = 1u;  // (every writer stores the same word)
}

// a box whose fields are finite but whose rotation is not orthonormal (col::box_rotation_ok)?  *status != 0: there is one
static __global__ __launch_bounds__(256) void col_check_prims(const mi_icp_primitive* __restrict__ prims, int64_t np,
                                                             uint32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const mi_icp_primitive P = prims[i];
    if (P.type == MI_ICP_PRIMITIVE_BOX && col::primitive_finite(P) && !col::box_rotation_ok(P.transform)) *status = 1u;
}

static __global__ __launch_bounds__(256) void col_hit_flags(const int32_t* __restrict__ hit, int64_t n, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = hit[i] >= 0 ? 1u : 0u;
}

// the pairs: (enumerated, other) when the enumerated side is A, else (other, enumerated); an enumerated occupancy-grid
// voxel is named by its linear index
static __global__ __launch_bounds__(256) void col_emit_pairs(const int32_t* __restrict__ hit, const uint32_t* __restrict__ pos, int64_t n,
                                                            int enumerated_first, const int32_t* __restrict__ occ_index, int res,
                                                            int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || hit[i] < 0) return;
    const int32_t me = occ_index ? (int32_t)cube_index(res, occ_index[i * 3], occ_index[i * 3 + 1], occ_index[i * 3 + 2]) : (int32_t)i;
    const int64_t p = pos[i];
    out[p * 2] = enumerated_first ? me : hit[i];
    out[p * 2 + 1] = enumerated_first ? hit[i] : me;
}

// the caller's index of every distinct sorted key: the first of its run in the stable order
static __global__ __launch_bounds__(256) void col_run_heads(const uint32_t* __restrict__ order, const uint32_t* __restrict__ run_start,
                                                           int64_t nvox, uint32_t* __restrict__ perm) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < nvox) perm[v] = order[run_start[v]];
}

// ---- CreateVoxelGrid of a primitive whose translation is zero: idx -> (w, h, d), kept iff it collides with that cell
struct ColDense {
    int nw, nh, nd;
    int64_t total;
    float vs;
};

__device__ __forceinline__ void col_dense_key(const ColDense& D, int64_t idx, int32_t* k) {
    const int64_t hd = (int64_t)D.nh * D.nd;
    k[0] = (int32_t)(idx / hd) - D.nw / 2;
    k[1] = (int32_t)((idx % hd) / D.nd) - D.nh / 2;
    k[2] = (int32_t)(idx % D.nd) - D.nd / 2;
}

static __global__ __launch_bounds__(256) void col_voxelize_flags(mi_icp_primitive P, ColDense D, uint32_t* __restrict__ flags) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= D.total) return;
    int32_t k[3];
    col_dense_key(D, idx, k);
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = col::cell_lo(k[a], D.vs, 0.0f);
        hi[a] = col::cell_hi(k[a], D.vs, 0.0f);
    }
    flags[idx] = col::primitive_cell(P, lo, hi, 0.0f) ? 1u : 0u;
}

static __global__ __launch_bounds__(256) void col_voxelize_emit(ColDense D, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                                               int32_t* __restrict__ out_keys, float* __restrict__ out_colors) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= D.total || !flags[idx]) return;
    int32_t k[3];
    col_dense_key(D, idx, k);
    const int64_t p = pos[idx];
    for (int a = 0; a < 3; ++a) {
        out_keys[p * 3 + a] = k[a];
        out_colors[p * 3 + a] = 1.0f;
    }
}

}  // namespace mi
