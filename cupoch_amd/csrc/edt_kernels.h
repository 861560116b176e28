// edt_kernels.h -- geometry::DistanceTransform (geometry/distancetransform.{h,cu}): the exact Euclidean distance
// transform of a set of site cells in a dense res^3 grid.  include/mi_icp.h holds the contract.
//
// A cell is ONE 32-bit word, indexed (x*res + y)*res + z, z fastest: the nearest site's x | y << 10 | z << 20, bit 31
// set when no site has been seen (kEdtNone, all bits set: a cleared plane is one memset).  The distance is derived from
// it when it is read.  Two planes, 8 bytes per cell:
//   edt_seed_*   plane A is cleared, then every site stores its own word at its cell: every writer of a word stores the
//                same value, so there are no atomics and the outcome depends on the site SET alone
//   edt_pass_z   A -> B: per (x, y) column the nearer of the last site at or below z and the next one above (a tie goes
//                down).  One wave per column, 64 cells per step: a wave max-scan with a carry upwards, the column's words
//                kept in registers (16 steps at most), then a min-scan downwards
//   edt_pass<1>  along y, then edt_pass<0> along x, B -> B with A as the stack: one lane per line, neighbouring lanes on
//                neighbouring z, so each step of a walk reads a coalesced row.  edt_envelope.h builds the lower envelope
//                and sweeps it.  A stack node lives in A at its own cell: its place on the line is the site's coordinate
//                along the line, so that field of the word holds the link to the node below, bit 30 marking the bottom.
//   edt_query    the batched point query          edt_unpack  the whole plane as indices and / or distances
// No kernel here keeps an array that is indexed at run time.
#pragma once
#include "device_utils.h"
#include "edt_envelope.h"
#include "grid_rules.h"

namespace mi {

constexpr uint32_t kEdtNone = 0xffffffffu;
constexpr uint32_t kEdtBottom = 1u << 30;  // a node without a node below
constexpr int kEdtMaxRes = 1024;
constexpr int kEdtMaxSteps = kEdtMaxRes / kWave;

struct EdtGrid {
    uint32_t* a;  // seeds, then the stacks
    uint32_t* b;  // the transform
    int64_t n;    // res^3
    int res, h_res;
};

__device__ __forceinline__ uint32_t edt_pack(int x, int y, int z) { return (uint32_t)x | ((uint32_t)y << 10) | ((uint32_t)z << 20); }
__device__ __forceinline__ int edt_field(uint32_t w, int k) { return (int)((w >> (10 * k)) & 1023u); }

// the site's own word at its cell, or one more in *dropped (one atomic per wave with a cell outside; a count is the
// same in any order)
__device__ __forceinline__ void edt_seed_one(const EdtGrid& g, bool live, int x, int y, int z, unsigned long long* dropped) {
    const bool in = live && cube_inside(g.res, x, y, z);
    if (in) g.a[cube_index(g.res, x, y, z)] = edt_pack(x, y, z);
    const uint64_t out = __ballot(live && !in);
    if (out && lane_id() == (int)__builtin_ctzll(out)) atomicAdd(dropped, (unsigned long long)__builtin_popcountll(out));
}

static __global__ __launch_bounds__(256) void edt_seed_cells(EdtGrid g, const int32_t* __restrict__ cells, int64_t n,
                                                            unsigned long long* dropped) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    int x = 0, y = 0, z = 0;
    if (live) {
        x = cells[i * 3];
        y = cells[i * 3 + 1];
        z = cells[i * 3 + 2];
    }
    edt_seed_one(g, live, x, y, z, dropped);
}

// VoxelGrid keys: cell = floor(((float)key * vs + origin_grid - origin_dt) / vs) + h per axis, in that order, vs the
// transform's (the grid's equals it within FLT_EPSILON, or the call was refused)
static __global__ __launch_bounds__(256) void edt_seed_keys(EdtGrid g, const int32_t* __restrict__ keys, int64_t n, GridFrame grid,
                                                           GridFrame dt, unsigned long long* dropped) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    int c[3] = {0, 0, 0};
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float p = ((float)keys[i * 3 + k] * dt.vs + grid.origin[k]) - dt.origin[k];
            c[k] = floor_int(p / dt.vs) + g.h_res;
        }
    }
    edt_seed_one(g, live, c[0], c[1], c[2], dropped);
}

// an OccupancyGrid's occupied voxels: those of its bounds box
static __global__ __launch_bounds__(256) void edt_seed_occupied(EdtGrid g, const float* __restrict__ prob, GridBox b, float thres) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b.count) return;
    int x, y, z;
    box_voxel(b, t, &x, &y, &z);
    const int64_t idx = cube_index(g.res, x, y, z);
    if (occupied(prob[idx], thres)) g.a[idx] = edt_pack(x, y, z);
}

// inclusive max-scan upwards / min-scan downwards over the lanes of the wave
__device__ __forceinline__ int edt_wave_max_up(int v) {
    const int lane = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o, 64);
        if (lane >= o) v = max(v, y);
    }
    return v;
}
__device__ __forceinline__ int edt_wave_min_down(int v) {
    const int lane = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_down(v, o, 64);
        if (lane + o < 64) v = min(v, y);
    }
    return v;
}

static __global__ __launch_bounds__(256) void edt_pass_z(EdtGrid g) {
    const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= (int64_t)g.res * g.res) return;  // (the whole wave)
    const int lane = lane_id();
    const int64_t base = col * g.res;
    const int x = (int)(col / g.res), y = (int)(col % g.res);
    int last[kEdtMaxSteps];  // the last site at or below the cell, -1: none (indexed by unrolled loops only)
    int carry = -1;
#pragma unroll
    for (int k = 0; k < kEdtMaxSteps; ++k) {
        last[k] = -1;
        if (k * kWave < g.res) {
            const int z = k * kWave + lane;
            const bool site = z < g.res && !(g.a[base + z] >> 31);
            const int v = max(edt_wave_max_up(site ? z : -1), carry);
            last[k] = v;
            carry = __builtin_amdgcn_readlane(v, 63);
        }
    }
    constexpr int kFar = 1 << 20;
    carry = kFar;
#pragma unroll
    for (int k = kEdtMaxSteps - 1; k >= 0; --k) {
        if (k * kWave < g.res) {
            const int z = k * kWave + lane;
            const int lo = last[k];
            const int hi = min(edt_wave_min_down(lo == z ? z : kFar), carry);  // (a site is its own last site)
            carry = __builtin_amdgcn_readlane(hi, 0);
            if (z < g.res) {
                const int dl = lo >= 0 ? z - lo : kFar, dh = hi < kFar ? hi - z : kFar;
                const int zs = dl <= dh ? lo : hi;
                g.b[base + z] = (dl == kFar && dh == kFar) ? kEdtNone : edt_pack(x, y, zs);
            }
        }
    }
}

// One line of the pass along axis AXIS (1: y, with z done; 0: x, with y and z done).  `cell`: the line's first cell,
// `stride`: from one cell of the line to the next; c1, c2: the line's own y (AXIS 0 only) and z.
template <int AXIS>
struct EdtLine {
    uint32_t* plane;  // read by load, written by emit
    uint32_t* nodes;
    int64_t cell, stride;
    int c1, c2;
    static constexpr uint32_t kLinkMask = 1023u << (10 * AXIS);

    __device__ __forceinline__ uint32_t load(int j) const { return plane[cell + j * stride]; }
    __device__ __forceinline__ bool none(uint32_t w) const { return (w >> 31) != 0; }
    __device__ __forceinline__ int64_t g(uint32_t w) const {
        const int dz = c2 - edt_field(w, 2);
        const int dy = AXIS == 0 ? c1 - edt_field(w, 1) : 0;
        return (int64_t)(dy * dy + dz * dz);
    }
    __device__ __forceinline__ void push(int j, uint32_t w, int prev) const {
        nodes[cell + j * stride] = (w & ~kLinkMask & ~kEdtBottom) | (prev < 0 ? kEdtBottom : (uint32_t)prev << (10 * AXIS));
    }
    __device__ __forceinline__ uint32_t node(int j) const { return nodes[cell + j * stride]; }
    __device__ __forceinline__ int link(uint32_t nd) const { return (nd & kEdtBottom) ? -1 : edt_field(nd, AXIS); }
    __device__ __forceinline__ void emit(int i, int j, uint32_t nd) const {
        plane[cell + i * stride] = (nd & ~kLinkMask & ~kEdtBottom) | ((uint32_t)j << (10 * AXIS));
    }
    __device__ __forceinline__ void emit_none(int i) const { plane[cell + i * stride] = kEdtNone; }
};

template <int AXIS>
__global__ __launch_bounds__(256) void edt_pass(EdtGrid g) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t res = g.res;
    if (l >= res * res) return;
    EdtLine<AXIS> line;
    line.plane = g.b;
    line.nodes = g.a;
    const int hi = (int)(l / res), lo = (int)(l % res);  // AXIS 1: (x, z); AXIS 0: (y, z)
    line.cell = AXIS == 1 ? (int64_t)hi * res * res + lo : l;
    line.stride = AXIS == 1 ? res : res * res;
    line.c1 = hi;
    line.c2 = lo;
    const int top = edt_build(line, g.res);
    edt_sweep(line, g.res, top);
}

__device__ __forceinline__ float edt_distance(uint32_t w, int x, int y, int z, float vs) {
    if (w >> 31) return __builtin_inff();
    const int dx = x - edt_field(w, 0), dy = y - edt_field(w, 1), dz = z - edt_field(w, 2);
    return sqrtf((float)(dx * dx + dy * dy + dz * dz)) * vs;
}

__device__ __forceinline__ void edt_store_nearest(int32_t* __restrict__ o, int64_t i, uint32_t w) {
    const bool none = (w >> 31) != 0;
    o[i * 3] = none ? -1 : edt_field(w, 0);
    o[i * 3 + 1] = none ? -1 : edt_field(w, 1);
    o[i * 3 + 2] = none ? -1 : edt_field(w, 2);
}

// the cell of a point is floor((q - origin) / vs) + h per axis; outside the grid on any axis: NaN and (-1, -1, -1)
static __global__ __launch_bounds__(256) void edt_query(EdtGrid g, GridFrame f, const float* __restrict__ pts, int64_t n,
                                                       float* __restrict__ odist, int32_t* __restrict__ onear) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = cell_of(f, pts[i * 3], 0) + g.h_res;
    const int y = cell_of(f, pts[i * 3 + 1], 1) + g.h_res;
    const int z = cell_of(f, pts[i * 3 + 2], 2) + g.h_res;
    const bool in = cube_inside(g.res, x, y, z);
    const uint32_t w = in ? g.b[cube_index(g.res, x, y, z)] : kEdtNone;
    odist[i] = in ? edt_distance(w, x, y, z, f.vs) : __builtin_nanf("");
    if (onear) edt_store_nearest(onear, i, w);
}

static __global__ __launch_bounds__(256) void edt_unpack(EdtGrid g, float vs, int32_t* __restrict__ onear, float* __restrict__ odist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t w = g.b[i];
    const int z = (int)(i % g.res), y = (int)((i / g.res) % g.res), x = (int)(i / ((int64_t)g.res * g.res));
    if (onear) edt_store_nearest(onear, i, w);
    if (odist) odist[i] = edt_distance(w, x, y, z, vs);
}

}  // namespace mi
