// graph_kernels.h -- the kernels of geometry::Graph<3> (include/mi_icp.h "graph"; launcher: mi_graph.hip).
//
// The reference keeps a Graph as a LineSet whose lines are sorted by (first, second), with a CSR offset per node, and
// runs its single-source shortest path as a host loop of thrust calls: per relaxation round a for_each over the nodes,
// a reduce_by_key over the edges sorted by target, a for_each over the reduced nodes, a find and a count_if, each
// followed by a host wait.  Here:
//   construct        gr_check_lines, gr_edge_keys -> radix_sort_pairs (primitives.h) -> gr_gather_edges, gr_offsets
//   lattice          gr_lattice: every node writes its point, its offset and its <= 26 edges where they belong
//   set / remove     gr_match_edges: a listed edge finds its run in the sorted lines by binary search
//   search, small    gr_sssp_small: ONE workgroup, distances / flags / predecessors in LDS, edges streamed, to the end
//   search, large    gr_sssp_round per frontier round (node-parallel, byte flags), gr_prev_* for the predecessors
// Distances are non-negative floats, which order as their bit patterns: a relaxation is an unsigned atomicMin.
#pragma once
#include "device_utils.h"
#include "graph_rules.h"

namespace mi {

using graph::kInfBits;
using graph::kUnresolved;

// status bits of the checks
constexpr uint32_t kGrBadIndex = 1u, kGrBadWeight = 2u, kGrBadOffsets = 4u;

// The small regime's bounds (mi_icp_graph_sssp_limits).  Per node the one workgroup keeps a distance, a predecessor
// and a tier-2 candidate (4 bytes each) and two open flags (1 byte each): 14 bytes, 112 KiB at 8192 nodes of the CU's
// 160 KiB of LDS; 16384 nodes would need 224 KiB.  Every round streams all edges (12 bytes each) through that one CU,
// so they have to stay in the 4 MiB L2 of its XCD: 262144 edges are 3 MiB.
constexpr int kGrSmallNodes = 8192;
constexpr int kGrSmallEdges = 262144;
constexpr int kGrSmallThreads = 1024;
constexpr int kGrBatchRounds = 32;  // large regime: rounds launched between two looks at the counter

// ---- construct ----------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void gr_check_lines(const int32_t* __restrict__ lines, int64_t m, int64_t n,
                                                            uint32_t* __restrict__ status) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int64_t a = lines[e * 2], b = lines[e * 2 + 1];
    if (a < 0 || a >= n || b < 0 || b >= n) atomicOr(status, kGrBadIndex);
}

// key = first << bits | second (bits: enough for n - 1), value = the line's position; an index out of range gives key 0
static __global__ __launch_bounds__(256) void gr_edge_keys(const int32_t* __restrict__ lines, int64_t m, int64_t n, int bits,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int64_t a = lines[e * 2], b = lines[e * 2 + 1];
    const bool ok = a >= 0 && a < n && b >= 0 && b < n;
    keys[e] = ok ? (((uint64_t)a << bits) | (uint64_t)b) : 0ull;
    vals[e] = (uint32_t)e;
}

static __global__ __launch_bounds__(256) void gr_gather_edges(const uint32_t* __restrict__ order, int64_t m,
                                                             const int32_t* __restrict__ lines, const float* __restrict__ weights,
                                                             const float* __restrict__ colors, int32_t* __restrict__ olines,
                                                             float* __restrict__ oweights, float* __restrict__ ocolors) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= m) return;
    const int64_t e = order[p];
    olines[p * 2] = lines[e * 2];
    olines[p * 2 + 1] = lines[e * 2 + 1];
    if (weights) oweights[p] = weights[e];
    if (colors) {
        ocolors[p * 3] = colors[e * 3];
        ocolors[p * 3 + 1] = colors[e * 3 + 1];
        ocolors[p * 3 + 2] = colors[e * 3 + 2];
    }
}

// the first position whose line is not below (a, b) in lines sorted by (first, second)
__device__ __forceinline__ int64_t gr_lower_bound(const int32_t* __restrict__ lines, int64_t m, int32_t a, int32_t b) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t x = lines[mid * 2], y = lines[mid * 2 + 1];
        if (x < a || (x == a && y < b)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// offsets[v] = the first line whose first index is >= v, v = 0..n (offsets[n] = m)
static __global__ __launch_bounds__(256) void gr_offsets(const int32_t* __restrict__ lines, int64_t m, int64_t n,
                                                        int32_t* __restrict__ offsets) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v > n) return;
    offsets[v] = v == n ? (int32_t)m : (int32_t)gr_lower_bound(lines, m, (int32_t)v, INT32_MIN);
}

// ---- weights ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gr_distance(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    // (sqrtf: the correctly rounded one; __fsqrt_rn is the hardware's approximation here, one ulp off now and then)
    return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

static __global__ __launch_bounds__(256) void gr_weights_from_distance(const float* __restrict__ pts, int64_t n,
                                                                      const int32_t* __restrict__ lines, int64_t m,
                                                                      float* __restrict__ w, uint32_t* __restrict__ status) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int64_t a = lines[e * 2], b = lines[e * 2 + 1];
    if (a < 0 || a >= n || b < 0 || b >= n) {
        atomicOr(status, kGrBadIndex);
        return;
    }
    w[e] = gr_distance(pts[a * 3], pts[a * 3 + 1], pts[a * 3 + 2], pts[b * 3], pts[b * 3 + 1], pts[b * 3 + 2]);
}

static __global__ __launch_bounds__(256) void gr_node_distances(const float* __restrict__ pts, int64_t n, float qx, float qy,
                                                               float qz, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = gr_distance(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], qx, qy, qz);
}

// ---- lattice ------------------------------------------------------------------------------------------------------
struct GrLattice {
    int rx, ry, rz;
    float mn[3], step[3];
    int64_t n, m;
};

static __global__ __launch_bounds__(256) void gr_lattice(GrLattice L, float* __restrict__ pts, int32_t* __restrict__ lines,
                                                        float* __restrict__ w, int32_t* __restrict__ offsets) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.n) return;
    const int64_t yz = (int64_t)L.ry * L.rz;
    const int x = (int)(i / yz), y = (int)((i % yz) / L.rz), z = (int)(i % L.rz);
    const float px = __fadd_rn(L.mn[0], __fmul_rn((float)x, L.step[0]));
    const float py = __fadd_rn(L.mn[1], __fmul_rn((float)y, L.step[1]));
    const float pz = __fadd_rn(L.mn[2], __fmul_rn((float)z, L.step[2]));
    pts[i * 3] = px;
    pts[i * 3 + 1] = py;
    pts[i * 3 + 2] = pz;
    int64_t e = graph::lattice_edge_offset(x, y, z, L.rx, L.ry, L.rz);
    offsets[i] = (int32_t)e;
    if (i == L.n - 1) offsets[L.n] = (int32_t)L.m;
    for (int dx = -1; dx <= 1; ++dx) {
        const int nx = x + dx;
        if (nx < 0 || nx >= L.rx) continue;
        const float qx = __fadd_rn(L.mn[0], __fmul_rn((float)nx, L.step[0]));
        for (int dy = -1; dy <= 1; ++dy) {
            const int ny = y + dy;
            if (ny < 0 || ny >= L.ry) continue;
            const float qy = __fadd_rn(L.mn[1], __fmul_rn((float)ny, L.step[1]));
            for (int dz = -1; dz <= 1; ++dz) {
                const int nz = z + dz;
                if (nz < 0 || nz >= L.rz || (dx == 0 && dy == 0 && dz == 0)) continue;
                const float qz = __fadd_rn(L.mn[2], __fmul_rn((float)nz, L.step[2]));
                if (e < L.m) {  // (the closed form keeps e below m; a store never leaves the caller's room)
                    lines[e * 2] = (int32_t)i;
                    lines[e * 2 + 1] = (int32_t)(((int64_t)nx * L.ry + ny) * L.rz + nz);
                    w[e] = gr_distance(px, py, pz, qx, qy, qz);
                }
                ++e;
            }
        }
    }
}

// ---- SetEdgeWeights / RemoveEdges: a listed edge (and its reverse when undirected) finds its lines ------------------
// Entry t < k is edges[t], entry t >= k the reverse of edges[t - k].  lines are sorted (construct): the run of lines
// equal to the edge starts at its lower bound.  weights != null: the run's weights become `weight`; flags != null: its
// flags are cleared.  k searches of log2(m) steps against m searches of log2(k) and a sort of the list the other way.
static __global__ __launch_bounds__(256) void gr_match_edges(const int32_t* __restrict__ lines, int64_t m,
                                                            const int32_t* __restrict__ edges, int64_t k, int both,
                                                            float* __restrict__ weights, float weight,
                                                            uint32_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (both ? 2 * k : k)) return;
    const bool rev = t >= k;
    const int64_t j = rev ? t - k : t;
    const int32_t a = edges[j * 2 + (rev ? 1 : 0)], b = edges[j * 2 + (rev ? 0 : 1)];
    for (int64_t p = gr_lower_bound(lines, m, a, b); p < m && lines[p * 2] == a && lines[p * 2 + 1] == b; ++p) {
        if (weights) weights[p] = weight;
        if (flags) flags[p] = 0u;
    }
}

static __global__ __launch_bounds__(256) void gr_fill_u32(uint32_t* __restrict__ p, int64_t n, uint32_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

static __global__ __launch_bounds__(256) void gr_compact_edges(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                                              int64_t m, const int32_t* __restrict__ lines,
                                                              const float* __restrict__ weights, const float* __restrict__ colors,
                                                              int32_t* __restrict__ olines, float* __restrict__ oweights,
                                                              float* __restrict__ ocolors) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m || !flags[e]) return;
    const int64_t p = pos[e];
    olines[p * 2] = lines[e * 2];
    olines[p * 2 + 1] = lines[e * 2 + 1];
    if (weights) oweights[p] = weights[e];
    if (colors) {
        ocolors[p * 3] = colors[e * 3];
        ocolors[p * 3 + 1] = colors[e * 3 + 1];
        ocolors[p * 3 + 2] = colors[e * 3 + 2];
    }
}

// ---- the search ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool gr_weight_ok(float w) { return w >= 0.0f; }  // (+inf passes, NaN and negatives do not)

// SMALL REGIME: one workgroup, one launch.  The inputs are checked (weights, indices), the distances relaxed round by
// round until a round opens no node that could matter, the early end's mask applied, the predecessors found by tier 1
// and the tier-2 rounds, and dist / prev written.  *status != 0: nothing else is written.
static __global__ __launch_bounds__(kGrSmallThreads) void gr_sssp_small(const int32_t* __restrict__ lines,
                                                                        const float* __restrict__ weights, int n, int m,
                                                                        int start, int end, float* __restrict__ out_dist,
                                                                        int32_t* __restrict__ out_prev,
                                                                        uint32_t* __restrict__ status /*[0] status, [1] rounds, [2] tier-2 rounds*/) {
    __shared__ uint32_t dist[kGrSmallNodes];
    __shared__ int32_t prev[kGrSmallNodes];
    __shared__ int32_t cand[kGrSmallNodes];
    __shared__ uint8_t open[2][kGrSmallNodes];
    __shared__ uint32_t flag[2];
    const int tid = (int)threadIdx.x;
    if (tid < 2) flag[tid] = 0u;
    for (int v = tid; v < n; v += kGrSmallThreads) {
        dist[v] = kInfBits;
        prev[v] = kUnresolved;
        cand[v] = kUnresolved;
        open[0][v] = 0;
        open[1][v] = 0;
    }
    __syncthreads();
    uint32_t bad = 0u;
    for (int e = tid; e < m; e += kGrSmallThreads) {
        const int a = lines[e * 2], b = lines[e * 2 + 1];
        if (a < 0 || a >= n || b < 0 || b >= n) bad |= kGrBadIndex;
        if (!gr_weight_ok(weights[e])) bad |= kGrBadWeight;
    }
    if (bad) atomicOr(&flag[0], bad);
    if (tid == 0) {
        dist[start] = 0u;
        prev[start] = start;
        open[0][start] = 1;
    }
    __syncthreads();
    if (flag[0]) {
        if (tid == 0) status[0] = flag[0];
        return;
    }
    // ---- distances
    int cur = 0;
    uint32_t rounds = 0;
    for (;;) {
        for (int e = tid; e < m; e += kGrSmallThreads) {
            const int u = lines[e * 2];
            if (!open[cur][u]) continue;
            const int v = lines[e * 2 + 1];
            const uint32_t d = __float_as_uint(__fadd_rn(__uint_as_float(dist[u]), weights[e]));
            if (d < dist[v] && d < atomicMin(&dist[v], d)) {
                open[cur ^ 1][v] = 1;
                if (end < 0 || d <= dist[end]) flag[1] = 1u;  // (a node opened beyond the end's distance cannot lower anything that is kept)
            }
        }
        __syncthreads();
        const uint32_t more = flag[1];
        for (int v = tid; v < n; v += kGrSmallThreads) open[cur][v] = 0;
        __syncthreads();
        if (tid == 0) flag[1] = 0u;
        ++rounds;
        cur ^= 1;
        if (!more) break;
        __syncthreads();
    }
    __syncthreads();
    // ---- the early end: every entry beyond the end's distance is (+inf, -1)
    if (end >= 0) {
        const uint32_t lim = dist[end];
        __syncthreads();
        for (int v = tid; v < n; v += kGrSmallThreads)
            if (dist[v] > lim) dist[v] = kInfBits;
        __syncthreads();
    }
    // ---- tier 1
    for (int e = tid; e < m; e += kGrSmallThreads) {
        const int u = lines[e * 2], v = lines[e * 2 + 1];
        if (v == start) continue;
        const float du = __uint_as_float(dist[u]), dv = __uint_as_float(dist[v]);
        if (graph::tier1_ok(du, dv, __fadd_rn(du, weights[e]))) atomicMin(&prev[v], u);
    }
    __syncthreads();
    // ---- tier 2
    uint32_t rounds2 = 0;
    for (;;) {
        for (int e = tid; e < m; e += kGrSmallThreads) {
            const int u = lines[e * 2], v = lines[e * 2 + 1];
            if (prev[v] != kUnresolved || prev[u] == kUnresolved) continue;
            const float du = __uint_as_float(dist[u]), dv = __uint_as_float(dist[v]);
            if (graph::tier2_ok(du, dv, __fadd_rn(du, weights[e]))) atomicMin(&cand[v], u);
        }
        __syncthreads();
        for (int v = tid; v < n; v += kGrSmallThreads)
            if (cand[v] != kUnresolved) {
                prev[v] = cand[v];
                cand[v] = kUnresolved;
                flag[1] = 1u;
            }
        __syncthreads();
        const uint32_t more = flag[1];
        __syncthreads();
        if (tid == 0) flag[1] = 0u;
        if (!more) break;
        ++rounds2;
        __syncthreads();
    }
    for (int v = tid; v < n; v += kGrSmallThreads) {
        out_dist[v] = __uint_as_float(dist[v]);
        out_prev[v] = prev[v] == kUnresolved ? -1 : prev[v];
    }
    if (tid == 0) {
        status[0] = 0u;
        status[1] = rounds;
        status[2] = rounds2;
    }
}

// LARGE REGIME.  gr_sssp_check: weights, indices and offsets, once.
static __global__ __launch_bounds__(256) void gr_sssp_check(const int32_t* __restrict__ offsets, const int32_t* __restrict__ lines,
                                                           const float* __restrict__ weights, int64_t n, int64_t m,
                                                           uint32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t bad = 0u;
    if (i < m) {
        const int64_t a = lines[i * 2], b = lines[i * 2 + 1];
        if (a < 0 || a >= n || b < 0 || b >= n) bad |= kGrBadIndex;
        if (!gr_weight_ok(weights[i])) bad |= kGrBadWeight;
    }
    if (i < n) {
        const int64_t lo = offsets[i], hi = offsets[i + 1];
        if (lo < 0 || hi < lo || hi > m || (i == 0 && lo != 0) || (i == n - 1 && hi != m)) bad |= kGrBadOffsets;
    }
    if (bad) atomicOr(status, bad);
}

// dist = +inf, prev = unresolved, no node open; then the start.  ctl[0..2]: the rounds' ring of counters, ctl[3] the
// number of rounds that did work, ctl[4] unresolved nodes after a predecessor pass, ctl[5] nodes a pass resolved.
static __global__ __launch_bounds__(256) void gr_sssp_init(int64_t n, int start, uint32_t* __restrict__ dist, int32_t* __restrict__ prev,
                                                          uint8_t* __restrict__ open0, uint8_t* __restrict__ open1,
                                                          uint32_t* __restrict__ ctl) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < 8) ctl[v] = v == 2 ? 1u : 0u;  // (round 0 reads slot 2 as "the round before opened a node")
    if (v >= n) return;
    dist[v] = v == start ? 0u : kInfBits;
    prev[v] = v == start ? start : kUnresolved;
    open0[v] = v == start ? 1 : 0;
    open1[v] = 0;
}

// One frontier round r: every open node relaxes its out-edges.  Counter slots: (r + 2) % 3 what round r - 1 opened
// (zero: this round returns at once), r % 3 what this round opens, (r + 1) % 3 zeroed for the next round.
static __global__ __launch_bounds__(256) void gr_sssp_round(const int32_t* __restrict__ offsets, const int32_t* __restrict__ lines,
                                                           const float* __restrict__ weights, int64_t n, int r, int end,
                                                           uint32_t* __restrict__ dist, uint8_t* __restrict__ open_cur,
                                                           uint8_t* __restrict__ open_next, uint32_t* __restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[(r + 1) % 3] = 0u;
    if (ctl[(r + 2) % 3] == 0u) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&ctl[3], 1u);
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t opened = 0u;
    if (v < n && open_cur[v]) {
        open_cur[v] = 0;
        const float dv = __uint_as_float(__hip_atomic_load(&dist[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const int32_t lo = offsets[v], hi = offsets[v + 1];
        for (int32_t e = lo; e < hi; ++e) {
            const int32_t t = lines[(int64_t)e * 2 + 1];
            const uint32_t d = __float_as_uint(__fadd_rn(dv, weights[e]));
            if (d < __hip_atomic_load(&dist[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) && d < atomicMin(&dist[t], d)) {
                open_next[t] = 1;
                if (end < 0 || d <= __hip_atomic_load(&dist[end], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) opened = 1u;
            }
        }
    }
    if (__syncthreads_or((int)opened) && threadIdx.x == 0) atomicAdd(&ctl[r % 3], 1u);
}

static __global__ __launch_bounds__(256) void gr_sssp_mask(int64_t n, int end, uint32_t* __restrict__ dist, uint32_t* __restrict__ dist_out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint32_t d = dist[v];
    dist_out[v] = (end >= 0 && d > dist[end]) ? kInfBits : d;
}

// tier 1, edge-parallel, after the distances stand
static __global__ __launch_bounds__(256) void gr_prev_tier1(const int32_t* __restrict__ lines, const float* __restrict__ weights,
                                                           int64_t m, int start, const uint32_t* __restrict__ dist,
                                                           int32_t* __restrict__ prev) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int32_t u = lines[e * 2], v = lines[e * 2 + 1];
    if (v == start) return;
    const float du = __uint_as_float(dist[u]), dv = __uint_as_float(dist[v]);
    if (graph::tier1_ok(du, dv, __fadd_rn(du, weights[e]))) atomicMin(&prev[v], u);
}

// commits the candidates of a tier-2 pass (none after tier 1) and counts: ctl[4] reachable nodes still unresolved,
// ctl[5] nodes resolved by this commit
static __global__ __launch_bounds__(256) void gr_prev_commit(int64_t n, const uint32_t* __restrict__ dist, int32_t* __restrict__ prev,
                                                            int32_t* __restrict__ cand, uint32_t* __restrict__ ctl) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t left = 0u, done = 0u;
    if (v < n) {
        if (cand[v] != kUnresolved) {
            prev[v] = cand[v];
            cand[v] = kUnresolved;
            done = 1u;
        } else if (prev[v] == kUnresolved && dist[v] != kInfBits) {
            left = 1u;
        }
    }
    const int nleft = __syncthreads_count((int)left), ndone = __syncthreads_count((int)done);
    if (threadIdx.x == 0) {
        if (nleft) atomicAdd(&ctl[4], (uint32_t)nleft);
        if (ndone) atomicAdd(&ctl[5], (uint32_t)ndone);
    }
}

static __global__ __launch_bounds__(256) void gr_prev_tier2(const int32_t* __restrict__ lines, const float* __restrict__ weights,
                                                           int64_t m, const uint32_t* __restrict__ dist,
                                                           const int32_t* __restrict__ prev, int32_t* __restrict__ cand) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const int32_t u = lines[e * 2], v = lines[e * 2 + 1];
    if (prev[v] != kUnresolved || prev[u] == kUnresolved) return;
    const float du = __uint_as_float(dist[u]), dv = __uint_as_float(dist[v]);
    if (graph::tier2_ok(du, dv, __fadd_rn(du, weights[e]))) atomicMin(&cand[v], u);
}

static __global__ __launch_bounds__(256) void gr_prev_finish(int64_t n, int32_t* __restrict__ prev) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n && prev[v] == kUnresolved) prev[v] = -1;
}

}  // namespace mi
