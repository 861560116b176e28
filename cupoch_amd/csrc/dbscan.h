// dbscan.h -- PointCloud::ClusterDBSCAN (geometry/pointcloud_cluster.cu:109-179) after its rows: the graph and the labels.
//
// The reference runs a host loop over the points: every point no earlier BFS reached starts one, each BFS level is a
// find plus a pass over the whole cloud, and each start ends with an n-int copy to the host.  Here, with the rows of
// knn_normals_kernel<4> (rows[i][0, deg(i)) = N(i), word[i] = deg(i) | kDbscanRowFull when the row may be truncated):
//   a. union-find over the MUTUAL core-core edges (i -> j and j -> i; j -> i needs no look when j's row is not full,
//      as d2 is symmetric in fp32): dbscan_hook hooks the larger root under the smaller with atomicCAS, dbscan_flatten
//      points every entry at its root, so rep[v] = the smallest index of v's piece.  Every piece is strongly connected.
//   b. dbscan_classify marks every other edge of a core point -- core -> non-core, and core -> core one way only --
//      in a 128-bit mask per row.  dbscan_round then propagates over those one-way edges, one value per piece:
//        phase 0: m = the smallest index that reaches the piece (atomicMin; initially the representative).  The
//                 representative is a ROOT iff its m equals it (no smaller point reaches it: the reference's loop
//                 starts a BFS there);
//        phase 1: M = the largest root that reaches the piece (atomicMax; the piece's own representative when that is
//                 a root).
//      A round that changes nothing ends its phase (dbscan_step).  Without truncated rows the only one-way edges lead
//      into non-core points, which have none of their own: each phase settles in one round plus one that checks.
//   c. a root starts a cluster iff |reach| >= min_points -- every core root, and an isolated point when
//      min_points <= 1; exclusive_scan_u32 over those flags numbers the clusters in ascending order of their roots,
//      and label(x) = number(M(x)), or -1 when M(x) started none (the BFS that reached x last is M(x)'s).
// Every value is the fixed point of min / max updates: the same bytes on every run and every context.
// The rounds are launched in batches and gated on the device (a settled phase returns at once), so the common case
// waits on the stream once; the host bounds the rounds by 2 * (one-way edges + 1) and fails past that.
//
// Memory on top of the cloud's tree: the rows, n * (max_edges + 1) int32 (4.04 GB at n = 10M, max_edges = 100), and
// 48 bytes per point (word, rep, m, M, start flag, cluster number, the 16-byte mask).
#pragma once
#include "device_utils.h"
#include "knn_normals.h"

namespace mi {

struct DbscanState {
    uint32_t phase;    // 0: m rounds, 1: M rounds, 2: settled
    uint32_t changed;  // the present round changed a value
    uint32_t rounds;   // rounds run while not settled
    uint32_t oneway;   // one-way edges (dbscan_classify)
};

__device__ __forceinline__ int32_t dbs_ld(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void dbs_st(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int dbs_deg(int32_t w) { return w & (kDbscanRowFull - 1); }
// the state words are read with vector loads from the L2, where the rounds' stores went
__device__ __forceinline__ uint32_t dbs_word(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v's tree; parent[] only ever points to a smaller index, so the walk ends.  Intermediate pointer jumping:
// every node passed is re-pointed at its grandparent (still an ancestor in the same piece).
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t v) {
    int32_t cur = dbs_ld(parent + v);
    if (cur != v) {
        int32_t prev = v, next;
        while (cur > (next = dbs_ld(parent + cur))) {
            dbs_st(parent + prev, next);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

// is i in N(j)?  A row that is not full holds every point within eps of j, i among them (d2 is symmetric).
__device__ __forceinline__ bool dbs_mutual(const int32_t* __restrict__ rows, int k, int32_t wj, int64_t j, int32_t i) {
    if (!(wj & kDbscanRowFull)) return true;
    const int32_t* row = rows + j * k;
    const int dj = dbs_deg(wj);
    for (int e = 0; e < dj; ++e)
        if (row[e] == i) return true;
    return false;
}

static __global__ __launch_bounds__(256) void dbscan_init(int64_t n, int32_t* __restrict__ parent, int32_t* __restrict__ m,
                                                          int32_t* __restrict__ Mx) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    parent[v] = (int32_t)v;
    m[v] = (int32_t)v;
    Mx[v] = -1;
}

// a. every mutual core-core edge i -> j with i < j (its twin j -> i is the same edge) joins the two pieces: the larger
// root is hooked under the smaller.  A failed CAS means the root got a parent meanwhile: go on from that (smaller) one.
static __global__ __launch_bounds__(256) void dbscan_hook(const int32_t* __restrict__ rows, const int32_t* __restrict__ word,
                                                          int64_t n, int k, int min_points, int32_t* parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int di = dbs_deg(word[i]);
    if (di < min_points) return;
    const int32_t* row = rows + i * k;
    for (int e = 0; e < di; ++e) {
        const int32_t j = row[e];
        if (j < i) continue;
        const int32_t wj = word[j];
        if (dbs_deg(wj) < min_points || !dbs_mutual(rows, k, wj, j, (int32_t)i)) continue;
        int32_t a = uf_find(parent, (int32_t)i), b = uf_find(parent, j);
        while (a != b) {  // each failed CAS lowers a root: at most i + j turns
            if (a > b) {
                const int32_t t = a;
                a = b;
                b = t;
            }
            const int32_t old = atomicCAS(parent + b, b, a);
            if (old == b) break;
            b = uf_find(parent, old);
        }
    }
}

// After the hooks: every entry becomes its root.  The walk only reads -- pointer jumping here could write a node's
// old grandparent over the root another thread has just stored there -- and each thread writes its own entry alone.
static __global__ __launch_bounds__(256) void dbscan_flatten(int64_t n, int32_t* parent) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    int32_t cur = dbs_ld(parent + v), next;
    while (cur > (next = dbs_ld(parent + cur))) cur = next;
    dbs_st(parent + v, cur);
}

// b. the one-way edges of every core point (those to non-core points, and to core points whose rows do not hold it),
// bit e of mask[i] for rows[i][e]; edges inside one piece carry nothing and are left out.  Their number goes to
// state->oneway (the bound on the rounds).
static __global__ __launch_bounds__(256) void dbscan_classify(const int32_t* __restrict__ rows,
                                                              const int32_t* __restrict__ word,
                                                              const int32_t* __restrict__ rep, int64_t n, int k,
                                                              int min_points, uint4* __restrict__ mask,
                                                              DbscanState* state) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t b[4] = {0u, 0u, 0u, 0u};
    const int di = dbs_deg(word[i]);
    uint32_t cnt = 0u;
    if (di >= min_points) {
        const int32_t* row = rows + i * k;
        const int32_t ri = rep[i];
        for (int e = 0; e < di; ++e) {
            const int32_t j = row[e];
            const int32_t wj = word[j];
            if (rep[j] == ri) continue;
            if (dbs_deg(wj) >= min_points && dbs_mutual(rows, k, wj, j, (int32_t)i)) continue;
            b[e >> 5] |= 1u << (e & 31);
            ++cnt;
        }
    }
    mask[i] = make_uint4(b[0], b[1], b[2], b[3]);
    if (cnt) atomicAdd(&state->oneway, cnt);
}

// M of piece p: what reached it, or p itself when p is a root
__device__ __forceinline__ int32_t dbs_M(const int32_t* m, const int32_t* Mx, int32_t p) {
    const int32_t own = dbs_ld(m + p) == p ? p : -1;
    return max(dbs_ld(Mx + p), own);
}

// One round over the one-way edges, of the phase state->phase says (none once settled).
static __global__ __launch_bounds__(256) void dbscan_round(const int32_t* __restrict__ rows, const uint4* __restrict__ mask,
                                                           const int32_t* __restrict__ rep, int64_t n, int k, int32_t* m,
                                                           int32_t* Mx, DbscanState* state) {
    const uint32_t phase = dbs_word(&state->phase);
    if (phase >= 2u) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4 mk = mask[i];
    if ((mk.x | mk.y | mk.z | mk.w) == 0u) return;
    const uint32_t bw[4] = {mk.x, mk.y, mk.z, mk.w};
    const int32_t* row = rows + i * k;
    const int32_t src = rep[i];
    bool changed = false;
    if (phase == 0u) {
        const int32_t v = dbs_ld(m + src);
        for (int w = 0; w < 4; ++w)
            for (uint32_t bits = bw[w]; bits; bits &= bits - 1u) {
                const int32_t d = rep[row[w * 32 + __builtin_ctz(bits)]];
                if (dbs_ld(m + d) > v && atomicMin(m + d, v) > v) changed = true;
            }
    } else {
        const int32_t v = dbs_M(m, Mx, src);
        for (int w = 0; w < 4; ++w)
            for (uint32_t bits = bw[w]; bits; bits &= bits - 1u) {
                const int32_t d = rep[row[w * 32 + __builtin_ctz(bits)]];
                if (dbs_ld(Mx + d) < v && atomicMax(Mx + d, v) < v) changed = true;
            }
    }
    if (changed) __hip_atomic_store(&state->changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// between two rounds: a round that changed nothing ends its phase
static __global__ __launch_bounds__(64) void dbscan_step(DbscanState* state) {
    if (threadIdx.x != 0) return;
    const uint32_t phase = dbs_word(&state->phase);
    if (phase >= 2u) return;
    state->rounds = dbs_word(&state->rounds) + 1u;
    if (!dbs_word(&state->changed)) state->phase = phase + 1u;
    state->changed = 0u;
}

// c. the roots that start a cluster (once settled)
static __global__ __launch_bounds__(256) void dbscan_starts(const int32_t* __restrict__ word, const int32_t* __restrict__ rep,
                                                            const int32_t* __restrict__ m, int64_t n, int min_points,
                                                            const DbscanState* state, uint32_t* __restrict__ start) {
    if (dbs_word(&state->phase) != 2u) return;
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const bool root = rep[x] == (int32_t)x && m[x] == (int32_t)x;
    start[x] = (root && (dbs_deg(word[x]) >= min_points || min_points <= 1)) ? 1u : 0u;
}

// label(x) = the number of M(x)'s cluster, or -1; degrees (may be null) = deg(x)
static __global__ __launch_bounds__(256) void dbscan_labels(const int32_t* __restrict__ word, const int32_t* __restrict__ rep,
                                                            const int32_t* __restrict__ m, const int32_t* __restrict__ Mx,
                                                            const uint32_t* __restrict__ start,
                                                            const uint32_t* __restrict__ number, int64_t n,
                                                            const DbscanState* state, int32_t* __restrict__ labels,
                                                            int32_t* __restrict__ degrees) {
    if (dbs_word(&state->phase) != 2u) return;
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const int32_t r = dbs_M(m, Mx, rep[x]);
    labels[x] = (r >= 0 && start[r]) ? (int32_t)number[r] : -1;  // (r >= 0 always: the smallest point reaching x is a root)
    if (degrees) degrees[x] = dbs_deg(word[x]);
}

}  // namespace mi
