// voxelgrid_kernels.h -- geometry::VoxelGrid (geometry/voxelgrid.cu, voxelgrid_factory.cu): a sparse voxel set as
// keys int32[m][3] + colours float[m][3], ascending lexicographically (x most significant).
//
// The reference: thrust::sort_by_key on Vector3i with reduce_by_key / unique_by_key behind it (fp32 colour sums in
// thrust's order), remove_if for the carvings, and one thrust::find -- a linear scan -- per query of CheckIfIncluded.
// Here every operation that has to bring equal keys together goes one way (mi_voxelgrid.hip vg_sort_runs):
//   vg_key_bounds_partial / _final   per-axis min and max of the keys, the number of keys that count
//   vg_pack<K>                       key - min packed into exactly the bits the extents need (K: 32 or 64 bits); a key
//                                    that does not count (a non-finite point) takes the x slot one past the largest
//   radix_sort_pairs<K>              stable: a run of equal keys stays in input order.  Extents that need more than
//                                    64 bits together: two stable sorts, (y, z) then x
//   vg_heads[_packed] + exclusive_scan_u32 + vg_run_starts[_packed]   the runs (from the packed keys where one key
//                                    holds the voxel, else from the keys themselves through the order)
// and what is made of a run differs: vg_run_color_means (fp64 mean of the run's colours), vg_merge_colors (operator+=:
// the fp32 sum left to right over the run length; AddVoxels: the run's first).  The carvings are flags + the scan + the
// gather of select.h; CheckIfIncluded is a binary search per query.  Nothing here takes an atomic on a shared word, and
// every sum has a fixed order.
#pragma once
#include "device_utils.h"
#include "grid_rules.h"

namespace mi {

constexpr int32_t kVgNoKey = INT32_MIN;  // x of a key that does not count (keys themselves stay inside +-1e9)
constexpr int kVgBlocks = 512;           // blocks of the partial reductions at most
constexpr uint32_t kVgThreadRun = 32u;   // runs up to this long are added up by one thread, longer ones by a wave

// create_from_pointcloud_functor (voxelgrid_factory.cu:67-72): floor((p - min_bound) / voxel_size) per axis, in fp32
static __global__ __launch_bounds__(256) void vg_point_keys(const float* __restrict__ xyz, int64_t n, GridFrame f,
                                                           int32_t* __restrict__ keys3) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    int32_t k[3] = {kVgNoKey, 0, 0};
    if (finite3(x, y, z)) {
        k[0] = cell_of(f, x, 0);
        k[1] = cell_of(f, y, 1);
        k[2] = cell_of(f, z, 2);
    }
    keys3[i * 3] = k[0];
    keys3[i * 3 + 1] = k[1];
    keys3[i * 3 + 2] = k[2];
}

// The fold of per-lane key bounds lo[3], hi[3] with either a count or (SUMS) fp64 sums s[3].  A wave: lane 0 leaves
// min[3], max[3] and the count in iout[0..7), the wave_sum lane the sums in dout[0..3).
template <bool SUMS>
__device__ __forceinline__ void vg_fold_wave(const int32_t* lo, const int32_t* hi, uint32_t cnt, const double* s,
                                             int32_t* iout, double* dout) {
    const int lane = lane_id();
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int32_t a = wave_min(lo[d]), b = wave_max(hi[d]);
        if (lane == 0) {
            iout[d] = a;
            iout[3 + d] = b;
        }
        if (SUMS) {
            const double t = wave_sum(s[d]);
            if (lane == kWaveSumLane) dout[d] = t;
        }
    }
    if (!SUMS) {
        const uint32_t t = wave_add(cnt);
        if (lane == 0) iout[6] = (int32_t)t;
    }
}

// The block's four waves, after a barrier behind their vg_fold_wave into ired[w] and dred[w]: the first WORDS (6, or 7
// with the count) of the fold to iout, the sums ((w0 + w1) + w2) + w3 to dout.
template <int WORDS, int STRIDE>
__device__ __forceinline__ void vg_fold_block(const int32_t (*ired)[STRIDE], const double (*dred)[3], int32_t* iout, double* dout) {
    const int d = (int)threadIdx.x;
    if (d < WORDS) {
        int32_t v = ired[0][d];
        for (int w = 1; w < 4; ++w) {
            if (d < 3) v = min(v, ired[w][d]);
            else if (d < 6) v = max(v, ired[w][d]);
            else v = (int32_t)((uint32_t)v + (uint32_t)ired[w][d]);
        }
        iout[d] = v;
    }
    if (dred && d < 3) dout[d] = ((dred[0][d] + dred[1][d]) + dred[2][d]) + dred[3][d];
}

// per block: min[3], max[3] of the keys that count, their number, a spare word -> part[block][8]
static __global__ __launch_bounds__(256) void vg_key_bounds_partial(const int32_t* __restrict__ keys3, int64_t n,
                                                                   int32_t* __restrict__ part) {
    __shared__ int32_t red[4][8];
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    uint32_t cnt = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t kx = keys3[i * 3];
        if (kx == kVgNoKey) continue;
        const int32_t k[3] = {kx, keys3[i * 3 + 1], keys3[i * 3 + 2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = min(lo[d], k[d]);
            hi[d] = max(hi[d], k[d]);
        }
        ++cnt;
    }
    vg_fold_wave<false>(lo, hi, cnt, nullptr, red[threadIdx.x >> 6], nullptr);
    __syncthreads();
    vg_fold_block<7>(red, nullptr, part + blockIdx.x * 8, nullptr);
}

static __global__ __launch_bounds__(64) void vg_key_bounds_final(const int32_t* __restrict__ part, int nblocks,
                                                                int32_t* __restrict__ out /*[8]*/) {
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    uint32_t cnt = 0u;
    for (int b = lane_id(); b < nblocks; b += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = min(lo[d], part[b * 8 + d]);
            hi[d] = max(hi[d], part[b * 8 + 3 + d]);
        }
        cnt += (uint32_t)part[b * 8 + 6];
    }
    vg_fold_wave<false>(lo, hi, cnt, nullptr, out, nullptr);
    if (lane_id() == 0) out[7] = 0;
}

// how key - lo is packed: x above y above z; nokey_x (the x extent) is the x slot of the keys that do not count, so
// they sort behind every other.  part: kVgWhole the whole key; kVgLow y and z only, kVgHigh x only -- the two stable
// sorts of keys whose extents need more than 64 bits together.
constexpr int kVgWhole = 0, kVgLow = 1, kVgHigh = 2;
struct VgPack {
    int32_t lo[3];
    int shift_x, shift_y;  // bits_y + bits_z, bits_z
    uint32_t nokey_x;
};

// keys[i] = the packed part of entry o = order ? order[i] : i, vals[i] = o (order may be vals itself: thread i reads
// and writes slot i only)
template <typename K>
static __global__ __launch_bounds__(256) void vg_pack(const int32_t* __restrict__ keys3, int64_t n, VgPack p, int part,
                                                     const uint32_t* order, K* __restrict__ keys, uint32_t* vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t o = order ? (int64_t)order[i] : i;
    const int32_t kx = keys3[o * 3];
    const bool counts = kx != kVgNoKey;
    const uint32_t rx = counts ? (uint32_t)kx - (uint32_t)p.lo[0] : p.nokey_x;
    const uint32_t ry = counts ? (uint32_t)keys3[o * 3 + 1] - (uint32_t)p.lo[1] : 0u;
    const uint32_t rz = counts ? (uint32_t)keys3[o * 3 + 2] - (uint32_t)p.lo[2] : 0u;
    K key;
    if (part == kVgHigh) key = (K)rx;
    else if (part == kVgLow) key = (K)(((uint64_t)ry << p.shift_y) | (uint64_t)rz);
    else key = (K)(((uint64_t)rx << p.shift_x) | ((uint64_t)ry << p.shift_y) | (uint64_t)rz);
    keys[i] = key;
    vals[i] = (uint32_t)o;
}

__device__ __forceinline__ bool vg_same_key(const int32_t* __restrict__ keys3, int64_t a, int64_t b) {
    return keys3[a * 3] == keys3[b * 3] && keys3[a * 3 + 1] == keys3[b * 3 + 1] && keys3[a * 3 + 2] == keys3[b * 3 + 2];
}

// head[i] = 1 where sorted element i counts and opens a run (the keys themselves are compared, through the order)
static __global__ __launch_bounds__(256) void vg_heads(const int32_t* __restrict__ keys3, const uint32_t* __restrict__ order,
                                                      int64_t n, uint32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t o = order[i];
    const bool counts = keys3[o * 3] != kVgNoKey;
    head[i] = (counts && (i == 0 || !vg_same_key(keys3, o, (int64_t)order[i - 1]))) ? 1u : 0u;
}

// run_start[r] = first sorted position of run r; run_start[number of runs] = the position behind the last key that
// counts (pos: the exclusive scan of head; the keys that do not count are sorted behind all others)
static __global__ __launch_bounds__(256) void vg_run_starts(const int32_t* __restrict__ keys3, const uint32_t* __restrict__ order,
                                                           const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos,
                                                           int64_t n, uint32_t* __restrict__ run_start) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = head[i];
    const bool counts = keys3[(int64_t)order[i] * 3] != kVgNoKey;
    if (h) run_start[pos[i]] = (uint32_t)i;
    if (!counts) {
        if (i == 0 || keys3[(int64_t)order[i - 1] * 3] != kVgNoKey) run_start[pos[i]] = (uint32_t)i;
    } else if (i == n - 1) {
        run_start[pos[i] + h] = (uint32_t)n;
    }
}

// the same two from the sorted PACKED keys, where one key holds the whole voxel (extents of up to 64 bits): no gathers
template <typename K>
static __global__ __launch_bounds__(256) void vg_heads_packed(const K* __restrict__ keys, int64_t n, VgPack p,
                                                             uint32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const K k = keys[i];
    const bool counts = (uint32_t)(k >> p.shift_x) != p.nokey_x;
    head[i] = (counts && (i == 0 || k != keys[i - 1])) ? 1u : 0u;
}

template <typename K>
static __global__ __launch_bounds__(256) void vg_run_starts_packed(const K* __restrict__ keys, const uint32_t* __restrict__ head,
                                                                  const uint32_t* __restrict__ pos, int64_t n, VgPack p,
                                                                  uint32_t* __restrict__ run_start) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = head[i];
    const bool counts = (uint32_t)(keys[i] >> p.shift_x) != p.nokey_x;
    if (h) run_start[pos[i]] = (uint32_t)i;
    if (!counts) {
        if (i == 0 || (uint32_t)(keys[i - 1] >> p.shift_x) != p.nokey_x) run_start[pos[i]] = (uint32_t)i;
    } else if (i == n - 1) {
        run_start[pos[i] + h] = (uint32_t)n;
    }
}

// the key of every run: that of its first element
static __global__ __launch_bounds__(256) void vg_emit_keys(const int32_t* __restrict__ keys3, const uint32_t* __restrict__ order,
                                                          const uint32_t* __restrict__ run_start, int64_t nvox,
                                                          int32_t* __restrict__ out_keys) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvox) return;
    const int64_t o = order[run_start[v]];
    out_keys[v * 3] = keys3[o * 3];
    out_keys[v * 3 + 1] = keys3[o * 3 + 1];
    out_keys[v * 3 + 2] = keys3[o * 3 + 2];
}

// The colour of every voxel: the fp64 mean of its points' colours, rounded once (colors == nullptr: (1, 1, 1)).  A
// thread per run adds a run of up to kVgThreadRun points in the run's order -- the input order, the sort is stable.
// The longer runs among a wave's 64 are then taken one after the other by the whole wave: lane l adds elements l,
// l + 64, ... in order and wave_sum adds the lanes in its fixed order, so one voxel that holds a whole cloud is read 64
// wide and the result is the same on every run (it may differ from the input-order sum in the last bit of the fp64
// sum, which the rounding to fp32 almost never sees).
static __global__ __launch_bounds__(256) void vg_run_color_means(const float* __restrict__ colors, const uint32_t* __restrict__ order,
                                                                const uint32_t* __restrict__ run_start, int64_t nvox,
                                                                float* __restrict__ out_colors) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = v < nvox;
    if (!colors) {
        if (live) {
            out_colors[v * 3] = 1.0f;
            out_colors[v * 3 + 1] = 1.0f;
            out_colors[v * 3 + 2] = 1.0f;
        }
        return;
    }
    const uint32_t s = live ? run_start[v] : 0u, e = live ? run_start[v + 1] : 0u;
    const uint32_t len = e - s;
    if (live && len <= kVgThreadRun) {
        double a[3] = {0.0, 0.0, 0.0};
        for (uint32_t t = s; t < e; ++t) {
            const int64_t o = order[t];
            a[0] += (double)colors[o * 3];
            a[1] += (double)colors[o * 3 + 1];
            a[2] += (double)colors[o * 3 + 2];
        }
        const double cnt = (double)len;
#pragma unroll
        for (int d = 0; d < 3; ++d) out_colors[v * 3 + d] = (float)(a[d] / cnt);
    }
    const int lane = lane_id();
    uint64_t longs = __ballot(live && len > kVgThreadRun);  // (wave-uniform from here on)
    while (longs != 0ull) {
        const int src = (int)__builtin_ctzll(longs);
        longs &= longs - 1ull;
        const uint32_t rs = (uint32_t)__shfl((int)s, src, 64), re = (uint32_t)__shfl((int)e, src, 64);
        double a[3] = {0.0, 0.0, 0.0};
        for (uint32_t t = rs + (uint32_t)lane; t < re; t += 64u) {
            const int64_t o = order[t];
            a[0] += (double)colors[o * 3];
            a[1] += (double)colors[o * 3 + 1];
            a[2] += (double)colors[o * 3 + 2];
        }
        const double cnt = (double)(re - rs);
        const int64_t vr = v - lane + src;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double sum = wave_sum(a[d]);
            if (lane == kWaveSumLane) out_colors[vr * 3 + d] = (float)(sum / cnt);
        }
    }
}

constexpr int kVgAverage = 0, kVgKeepFirst = 1;  // MI_ICP_VOXELGRID_AVERAGE / _KEEP_FIRST

// operator+= (voxelgrid.cu:254-277): the fp32 sum of the run's colours, left to right in the stable order (A's entries
// before B's, each side in its own order), over the run length in fp32.  AddVoxel / AddVoxels: the run's first entry.
static __global__ __launch_bounds__(256) void vg_merge_colors(const float* __restrict__ colors, const uint32_t* __restrict__ order,
                                                             const uint32_t* __restrict__ run_start, int64_t nvox, int mode,
                                                             float* __restrict__ out_colors) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvox) return;
    const uint32_t s = run_start[v], e = run_start[v + 1];
    int64_t o = order[s];
    float a[3] = {colors[o * 3], colors[o * 3 + 1], colors[o * 3 + 2]};
    if (mode == kVgAverage) {
        for (uint32_t t = s + 1u; t < e; ++t) {
            o = order[t];
            a[0] += colors[o * 3];
            a[1] += colors[o * 3 + 1];
            a[2] += colors[o * 3 + 2];
        }
        const float cnt = (float)(e - s);
#pragma unroll
        for (int d = 0; d < 3; ++d) a[d] = a[d] / cnt;
    }
    out_colors[v * 3] = a[0];
    out_colors[v * 3 + 1] = a[1];
    out_colors[v * 3 + 2] = a[2];
}

// CreateDense (voxelgrid_factory.cu:42-55): idx -> (idx / (h d), (idx % (h d)) / d, idx % d), colour (1, 1, 1)
static __global__ __launch_bounds__(256) void vg_dense(int64_t total, int num_h, int num_d, int32_t* __restrict__ out_keys,
                                                      float* __restrict__ out_colors) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t hd = (int64_t)num_h * num_d;
    const int64_t r = i % hd;
    out_keys[i * 3] = (int32_t)(i / hd);
    out_keys[i * 3 + 1] = (int32_t)(r / num_d);
    out_keys[i * 3 + 2] = (int32_t)(r % num_d);
    out_colors[i * 3] = 1.0f;
    out_colors[i * 3 + 1] = 1.0f;
    out_colors[i * 3 + 2] = 1.0f;
}

struct VgCamera {
    float K[9];  // row-major, the zeros included
    float R[9];  // row-major
    float t[3];
    int width, height;
    int float_image;  // 1 channel x 4 bytes: anything else is never "within"
    int keep_outside;
};

// compute_carve_functor (voxelgrid.cu:58-123) in fp32, unfused, in the reference's order; FloatValueAt is image.h:240-264.
// flags[i] = 1: voxel i stays.
static __global__ __launch_bounds__(256) void vg_carve_flags(const int32_t* __restrict__ keys, int64_t m, GridFrame f, VgCamera cam,
                                                            const float* __restrict__ image, uint32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const float r = f.vs / 2.0f;
    float c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = ((float)keys[i * 3 + d] + 0.5f) * f.vs + f.origin[d];
    bool stay = false;
    // GetVoxelBoundingPoints' order: (-,-,-) (-,-,+) (+,-,-) (+,-,+) (-,+,-) (-,+,+) (+,+,-) (+,+,+)
    for (int q = 0; q < 8 && !stay; ++q) {
        const float p[3] = {c[0] + ((q & 2) ? r : -r), c[1] + ((q & 4) ? r : -r), c[2] + ((q & 1) ? r : -r)};
        float X[3], uvz[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) X[d] = ((cam.R[d * 3] * p[0] + cam.R[d * 3 + 1] * p[1]) + cam.R[d * 3 + 2] * p[2]) + cam.t[d];
#pragma unroll
        for (int d = 0; d < 3; ++d) uvz[d] = (cam.K[d * 3] * X[0] + cam.K[d * 3 + 1] * X[1]) + cam.K[d * 3 + 2] * X[2];
        const float z = uvz[2];
        const float u = uvz[0] / z, v = uvz[1] / z;
        // (a NaN u or v fails the first two comparisons' negation: not within)
        const bool within = cam.float_image && u >= 0.0f && u <= (float)(cam.width - 1) && v >= 0.0f && v <= (float)(cam.height - 1);
        if (!within) {
            stay = cam.keep_outside != 0;
            continue;
        }
        const int ui = max(min((int)u, cam.width - 2), 0);
        const int vi = max(min((int)v, cam.height - 2), 0);
        const float pu = u - (float)ui, pv = v - (float)vi;
        const float v00 = image[(int64_t)vi * cam.width + ui], v01 = image[(int64_t)(vi + 1) * cam.width + ui];
        const float v10 = image[(int64_t)vi * cam.width + ui + 1], v11 = image[(int64_t)(vi + 1) * cam.width + ui + 1];
        const float dep = (v00 * (1.0f - pv) + v01 * pv) * (1.0f - pu) + (v10 * (1.0f - pv) + v11 * pv) * pu;
        stay = dep > 0.0f && z >= dep;
    }
    flags[i] = stay ? 1u : 0u;
}

// CheckIfIncluded (voxelgrid.cu:365-376): the voxel of a query is floor((q - origin) / voxel_size); it is included iff
// that key is among the ascending keys[m] -- a binary search.  A non-finite query is not included and has index (0, 0, 0).
static __global__ __launch_bounds__(256) void vg_query(const int32_t* __restrict__ keys, int64_t m, GridFrame f,
                                                      const float* __restrict__ queries, int64_t nq,
                                                      uint8_t* __restrict__ included, int32_t* __restrict__ out_index) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const float x = queries[i * 3], y = queries[i * 3 + 1], z = queries[i * 3 + 2];
    int32_t k[3] = {0, 0, 0};
    bool hit = false;
    if (finite3(x, y, z)) {
        k[0] = cell_of(f, x, 0);
        k[1] = cell_of(f, y, 1);
        k[2] = cell_of(f, z, 2);
        const int64_t lo = keys3_lower(keys, m, k[0], k[1], k[2]);
        hit = lo < m && keys[lo * 3] == k[0] && keys[lo * 3 + 1] == k[1] && keys[lo * 3 + 2] == k[2];
    }
    included[i] = hit ? 1 : 0;
    if (out_index) {
        out_index[i * 3] = k[0];
        out_index[i * 3 + 1] = k[1];
        out_index[i * 3 + 2] = k[2];
    }
}

// GetMinBound / GetMaxBound / GetCenter (voxelgrid.cu:161-200): per block the min and max index per axis and the fp64
// sum of the voxels' centres, each centre ((float)key * vs + origin) + 0.5f * vs in fp32.  ipart[block][8], dpart[block][4].
static __global__ __launch_bounds__(256) void vg_bounds_partial(const int32_t* __restrict__ keys, int64_t m, GridFrame f,
                                                               int32_t* __restrict__ ipart, double* __restrict__ dpart) {
    __shared__ int32_t ired[4][6];
    __shared__ double dred[4][3];
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    double s[3] = {0.0, 0.0, 0.0};
    const float half = 0.5f * f.vs;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int32_t k = keys[i * 3 + d];
            lo[d] = min(lo[d], k);
            hi[d] = max(hi[d], k);
            s[d] += (double)(((float)k * f.vs + f.origin[d]) + half);
        }
    }
    const int wid = (int)(threadIdx.x >> 6);
    vg_fold_wave<true>(lo, hi, 0u, s, ired[wid], dred[wid]);
    __syncthreads();
    vg_fold_block<6>(ired, dred, ipart + blockIdx.x * 8, dpart + blockIdx.x * 4);
}

static __global__ __launch_bounds__(64) void vg_bounds_final(const int32_t* __restrict__ ipart, const double* __restrict__ dpart,
                                                            int nblocks, int32_t* __restrict__ iout /*[6]*/,
                                                            double* __restrict__ dout /*[3]*/) {
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = lane_id(); b < nblocks; b += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = min(lo[d], ipart[b * 8 + d]);
            hi[d] = max(hi[d], ipart[b * 8 + 3 + d]);
            s[d] += dpart[b * 4 + d];
        }
    }
    vg_fold_wave<true>(lo, hi, 0u, s, iout, dout);
}

// PaintIndexedColor's indices: *status is set when one lies outside [0, m)
static __global__ __launch_bounds__(256) void vg_check_indices(const int64_t* __restrict__ idx, int64_t n_idx, int64_t m,
                                                              uint32_t* __restrict__ status) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_idx) return;
    const int64_t i = idx[j];
    if (i < 0 || i >= m) *status = 1u;  // (every writer stores the same word)
}

// PaintUniformColor (idx == nullptr: entries 0 .. count) / PaintIndexedColor (entries idx[0 .. count), checked before)
static __global__ __launch_bounds__(256) void vg_paint(float* __restrict__ colors, const int64_t* __restrict__ idx, int64_t count,
                                                      float r, float g, float b) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    const int64_t i = idx ? idx[j] : j;
    colors[i * 3] = r;
    colors[i * 3 + 1] = g;
    colors[i * 3 + 2] = b;
}

}  // namespace mi
