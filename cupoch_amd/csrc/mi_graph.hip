// mi_graph.hip -- geometry::Graph<3>: ConstructGraph, the lattice factory, the edge-weight and edge-removal updates and
// the single-source shortest path (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "graph_kernels.h"

#include <climits>

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// The contract is in include/mi_icp.h ("graph"), the kernels in graph_kernels.h, the rules host and device share in
// graph_rules.h.  Scratch: flags[0] the checks' status word, stage[0..2] the sorted / compacted lines, weights and
// colours before they go back to the caller's arrays, the sort buffers (keys0/1, vals0/1, hist, scan_tmp), dense_idx
// the compaction's positions; the search keeps its distances in stage[3], its candidates in stage[4], its two flag
// planes in stage[5] and its control words in bounds.

static int bits_for(int64_t n) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) < n) ++b;
    return b;
}

static int status_word(mi_icp_ctx* c, uint32_t** status) {
    TRY(ensure(c, c->flags, 1, status));
    HIPCHK(c, hipMemsetAsync(*status, 0, sizeof(uint32_t), c->stream));
    return MI_ICP_OK;
}

static int sizes_ok(mi_icp_ctx* c, const char* what, int64_t n_points, int64_t m) {
    TRY(count_ok(c, what, n_points));
    TRY(count_ok(c, what, m));
    return MI_ICP_OK;
}

static int write_offsets(mi_icp_ctx* c, const int32_t* lines, int64_t m, int64_t n_points, int32_t* offsets) {
    gr_offsets<<<blocks_for(n_points + 1), 256, 0, c->stream>>>(lines, m, n_points, offsets);
    KCHK(c);
    return MI_ICP_OK;
}

extern "C" {

int mi_icp_graph_construct(mi_icp_ctx* c, int32_t* lines, float* weights, float* colors, int64_t m, int64_t n_points,
                           int32_t* out_offsets) {
    const char* what = "graph_construct";
    TRY(check_ctx(c));
    TRY(sizes_ok(c, what, n_points, m));
    if (!out_offsets || (m > 0 && !lines)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    if (m == 0) {
        HIPCHK(c, hipMemsetAsync(out_offsets, 0, (size_t)(n_points + 1) * sizeof(int32_t), c->stream));
        return MI_ICP_OK;
    }
    uint32_t* status;
    TRY(status_word(c, &status));
    gr_check_lines<<<blocks_for(m), 256, 0, c->stream>>>(lines, m, n_points, status);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SortBuffers sb;
    TRY(sort_buffers(c, m, &sb));
    const int bits = bits_for(n_points);
    gr_edge_keys<<<blocks_for(m), 256, 0, c->stream>>>(lines, m, n_points, bits, sb.keys[0], sb.vals[0]);
    KCHK(c);
    const int cur = radix_sort_pairs<uint64_t>(c->stream, sb, m, 2 * bits);
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->u_host[0]) return fail(c, MI_ICP_ERR_INVALID, "%s: a line's point index is out of range [0, %lld)", what, (long long)n_points);
    int32_t* sl;
    float *sw = nullptr, *sc = nullptr;
    TRY(ensure(c, c->stage[0], (size_t)m * 2, &sl));
    if (weights) TRY(ensure(c, c->stage[1], (size_t)m, &sw));
    if (colors) TRY(ensure(c, c->stage[2], (size_t)m * 3, &sc));
    gr_gather_edges<<<blocks_for(m), 256, 0, c->stream>>>(sb.vals[cur], m, lines, weights, colors, sl, sw, sc);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(lines, sl, (size_t)m * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    if (weights) HIPCHK(c, hipMemcpyAsync(weights, sw, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (colors) HIPCHK(c, hipMemcpyAsync(colors, sc, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return write_offsets(c, lines, m, n_points, out_offsets);
}

int mi_icp_graph_weights_from_distance(mi_icp_ctx* c, const float* points, int64_t n_points, const int32_t* lines, int64_t m,
                                       float* out_weights) {
    const char* what = "graph_weights_from_distance";
    TRY(check_ctx(c));
    TRY(sizes_ok(c, what, n_points, m));
    if (m == 0) return MI_ICP_OK;
    if (!lines || !out_weights || !points) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    uint32_t* status;
    TRY(status_word(c, &status));
    gr_weights_from_distance<<<blocks_for(m), 256, 0, c->stream>>>(points, n_points, lines, m, out_weights, status);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->u_host[0]) return fail(c, MI_ICP_ERR_INVALID, "%s: a line's point index is out of range [0, %lld)", what, (long long)n_points);
    return MI_ICP_OK;
}

int mi_icp_graph_node_distances(mi_icp_ctx* c, const float* points, int64_t n_points, const float* point3, float* out_distances) {
    const char* what = "graph_node_distances";
    TRY(check_ctx(c));
    TRY(sizes_ok(c, what, n_points, 0));
    if (!point3) return fail(c, MI_ICP_ERR_INVALID, "%s: null point", what);
    if (n_points == 0) return MI_ICP_OK;
    if (!points || !out_distances) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    gr_node_distances<<<blocks_for(n_points), 256, 0, c->stream>>>(points, n_points, point3[0], point3[1], point3[2], out_distances);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_graph_lattice(mi_icp_ctx* c, const float* min3, const float* max3, const int32_t* resolutions3, float* out_points,
                         int64_t point_capacity, int32_t* out_lines, float* out_weights, int64_t edge_capacity,
                         int32_t* out_offsets, int64_t* n_points, int64_t* m) {
    const char* what = "graph_lattice";
    // (the counts are closed forms: they need no device, so a null context is turned away only when there is room to write)
    if (!n_points || !m) return fail(c, MI_ICP_ERR_INVALID, "%s: a count is null", what);
    *n_points = *m = 0;
    if (!min3 || !max3 || !resolutions3) return fail(c, MI_ICP_ERR_INVALID, "%s: null argument", what);
    if (point_capacity < 0 || edge_capacity < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative capacity", what);
    const int64_t rx = resolutions3[0], ry = resolutions3[1], rz = resolutions3[2];
    if (rx < 1 || ry < 1 || rz < 1) return fail(c, MI_ICP_ERR_INVALID, "%s: a resolution below 1", what);
    // (each factor is below 2^33, so the products are taken one at a time against the limit)
    if (rx * ry > (int64_t)INT_MAX || rx * ry * rz > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "%s: too many nodes", what);
    const int64_t n = rx * ry * rz;
    const double edges = (3.0 * rx - 2.0) * (3.0 * ry - 2.0) * (3.0 * rz - 2.0) - (double)n;
    if (edges > (double)INT_MAX) return fail(c, MI_ICP_ERR_INVALID, "%s: more than 2^31 - 1 edges", what);
    const int64_t cnt = graph::lattice_edge_count(rx, ry, rz);
    *n_points = n;
    *m = cnt;
    if (point_capacity < n || edge_capacity < cnt) return MI_ICP_OK;  // nothing is written: the caller learns the room to make
    TRY(check_ctx(c));
    if (!out_points || !out_offsets || (cnt > 0 && (!out_lines || !out_weights))) return fail(c, MI_ICP_ERR_INVALID, "%s: null output", what);
    GrLattice L;
    L.rx = (int)rx;
    L.ry = (int)ry;
    L.rz = (int)rz;
    L.n = n;
    L.m = cnt;
    for (int k = 0; k < 3; ++k) {
        L.mn[k] = min3[k];
        L.step[k] = (max3[k] - min3[k]) / (float)resolutions3[k];
    }
    gr_lattice<<<blocks_for(n), 256, 0, c->stream>>>(L, out_points, out_lines, out_weights, out_offsets);
    KCHK(c);
    return MI_ICP_OK;
}

// the two updates' common opening: sizes, buffers, the listed edges inside [0, n_points)
static int match_open(mi_icp_ctx* c, const char* what, const int32_t* lines, int64_t m, int64_t n_points, const int32_t* edges,
                      int64_t k) {
    TRY(check_ctx(c));
    TRY(sizes_ok(c, what, n_points, m));
    if (k < 0 || k > kMaxCount / 2) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if ((m > 0 && !lines) || (k > 0 && !edges)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    return MI_ICP_OK;
}

int mi_icp_graph_set_edge_weights(mi_icp_ctx* c, const int32_t* lines, float* weights, int64_t m, const int32_t* edges, int64_t k,
                                  int is_directed, float weight) {
    const char* what = "graph_set_edge_weights";
    TRY(match_open(c, what, lines, m, kMaxCount, edges, k));
    if (m == 0 || k == 0) return MI_ICP_OK;
    if (!weights) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const int both = is_directed ? 0 : 1;
    gr_match_edges<<<blocks_for(both ? 2 * k : k), 256, 0, c->stream>>>(lines, m, edges, k, both, weights, weight, nullptr);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_graph_remove_edges(mi_icp_ctx* c, int32_t* lines, float* weights, float* colors, int64_t m, int64_t n_points,
                              const int32_t* edges, int64_t k, int is_directed, int32_t* out_offsets, int64_t* m_out) {
    const char* what = "graph_remove_edges";
    if (!c) return MI_ICP_ERR_INVALID;
    if (!m_out) return fail(c, MI_ICP_ERR_INVALID, "%s: m_out is null", what);
    *m_out = 0;
    TRY(match_open(c, what, lines, m, n_points, edges, k));
    if (!out_offsets) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    if (m == 0) {
        HIPCHK(c, hipMemsetAsync(out_offsets, 0, (size_t)(n_points + 1) * sizeof(int32_t), c->stream));
        return MI_ICP_OK;
    }
    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)m, &flags));
    gr_fill_u32<<<blocks_for(m), 256, 0, c->stream>>>(flags, m, 1u);
    KCHK(c);
    const int both = is_directed ? 0 : 1;
    if (k > 0) {
        gr_match_edges<<<blocks_for(both ? 2 * k : k), 256, 0, c->stream>>>(lines, m, edges, k, both, nullptr, 0.0f, flags);
        KCHK(c);
    }
    TRY(scan_flags(c, flags, m, &pos, &total));
    TRY(read_total(c, total));
    int32_t* sl;
    float *sw = nullptr, *sc = nullptr;
    TRY(ensure(c, c->stage[0], (size_t)m * 2, &sl));
    if (weights) TRY(ensure(c, c->stage[1], (size_t)m, &sw));
    if (colors) TRY(ensure(c, c->stage[2], (size_t)m * 3, &sc));
    gr_compact_edges<<<blocks_for(m), 256, 0, c->stream>>>(flags, pos, m, lines, weights, colors, sl, sw, sc);
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t cnt = (int64_t)c->u_host[0];
    *m_out = cnt;
    if (cnt > 0) {
        HIPCHK(c, hipMemcpyAsync(lines, sl, (size_t)cnt * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        if (weights) HIPCHK(c, hipMemcpyAsync(weights, sw, (size_t)cnt * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        if (colors) HIPCHK(c, hipMemcpyAsync(colors, sc, (size_t)cnt * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    return write_offsets(c, lines, cnt, n_points, out_offsets);
}

int mi_icp_graph_sssp_limits(int64_t* small_max_nodes, int64_t* small_max_edges, int32_t* batch_rounds) {
    if (small_max_nodes) *small_max_nodes = kGrSmallNodes;
    if (small_max_edges) *small_max_edges = kGrSmallEdges;
    if (batch_rounds) *batch_rounds = kGrBatchRounds;
    return MI_ICP_OK;
}

int mi_icp_graph_sssp(mi_icp_ctx* c, const int32_t* offsets, const int32_t* lines, const float* weights, int64_t n, int64_t m,
                      int64_t start, int64_t end, float* out_dist, int32_t* out_prev, int32_t* info5) {
    const char* what = "graph_sssp";
    TRY(check_ctx(c));
    if (info5) std::memset(info5, 0, 5 * sizeof(int32_t));
    TRY(sizes_ok(c, what, n, m));
    if (n == 0) return fail(c, MI_ICP_ERR_INVALID, "%s: the graph has no node", what);
    if (start < 0 || start >= n) return fail(c, MI_ICP_ERR_INVALID, "%s: the start is out of range [0, %lld)", what, (long long)n);
    if (end >= n) return fail(c, MI_ICP_ERR_INVALID, "%s: the end is out of range [0, %lld)", what, (long long)n);
    if (end < 0) end = -1;
    if (!offsets || !out_dist || !out_prev || (m > 0 && (!lines || !weights))) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    auto refuse = [&](uint32_t st) {
        return fail(c, MI_ICP_ERR_INVALID, "%s: %s", what,
                    (st & kGrBadWeight) ? "a weight is negative or NaN"
                                        : ((st & kGrBadIndex) ? "a line's node index is out of range" : "the offsets do not partition the lines"));
    };
    uint32_t* ctl;
    TRY(ensure(c, c->bounds, 16, &ctl));
    if (n <= kGrSmallNodes && m <= kGrSmallEdges) {  // ---- small: one launch, one wait
        HIPCHK(c, hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), c->stream));
        gr_sssp_small<<<1, kGrSmallThreads, 0, c->stream>>>(lines, weights, (int)n, (int)m, (int)start, (int)end, out_dist, out_prev, ctl);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(c->u_host, ctl, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->u_host[0]) return refuse(c->u_host[0]);
        if (info5) {
            info5[0] = 0;
            info5[1] = 1;
            info5[2] = 1;
            info5[3] = (int32_t)c->u_host[1];
            info5[4] = (int32_t)c->u_host[2];
        }
        return MI_ICP_OK;
    }
    // ---- large: frontier rounds in batches, one counter read per batch
    uint32_t *status, *dist;
    int32_t* cand;
    uint8_t* open;
    TRY(status_word(c, &status));
    TRY(ensure(c, c->stage[3], (size_t)n, &dist));
    TRY(ensure(c, c->stage[4], (size_t)n, &cand));
    TRY(ensure(c, c->stage[5], (size_t)n * 2, &open));
    int launches = 0, waits = 0;
    gr_sssp_check<<<blocks_for(std::max(n, m)), 256, 0, c->stream>>>(offsets, lines, weights, n, m, status);
    KCHK(c);
    gr_sssp_init<<<blocks_for(std::max<int64_t>(n, 8)), 256, 0, c->stream>>>(n, (int)start, dist, out_prev, open, open + n, ctl);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the rounds walk the offsets: none is launched over a bad graph)
    ++waits;
    launches += 2;
    if (c->u_host[0]) return refuse(c->u_host[0]);
    int r = 0;
    for (;;) {
        for (int b = 0; b < kGrBatchRounds; ++b, ++r) {
            gr_sssp_round<<<blocks_for(n), 256, 0, c->stream>>>(offsets, lines, weights, n, r, (int)end, dist, open + (size_t)(r & 1) * n,
                                                             open + (size_t)((r + 1) & 1) * n, ctl);
            KCHK(c);
        }
        launches += kGrBatchRounds;
        HIPCHK(c, hipMemcpyAsync(c->u_host, ctl + ((r - 1) % 3), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->u_host + 1, ctl + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ++waits;
        if (c->u_host[0] == 0u) break;
        if ((int64_t)r > n + kGrBatchRounds) return fail(c, MI_ICP_ERR_STATE, "%s: the rounds did not end", what);  // (n rounds settle any graph)
    }
    const int32_t rounds = (int32_t)c->u_host[1];
    gr_sssp_mask<<<blocks_for(n), 256, 0, c->stream>>>(n, (int)end, dist, reinterpret_cast<uint32_t*>(out_dist));
    KCHK(c);
    const uint32_t* fdist = reinterpret_cast<const uint32_t*>(out_dist);
    gr_fill_u32<<<blocks_for(n), 256, 0, c->stream>>>(reinterpret_cast<uint32_t*>(cand), n, (uint32_t)kUnresolved);
    KCHK(c);
    if (m > 0) {
        gr_prev_tier1<<<blocks_for(m), 256, 0, c->stream>>>(lines, weights, m, (int)start, fdist, out_prev);
        KCHK(c);
    }
    launches += 3;
    int rounds2 = 0;
    for (int pass = 0;; ++pass) {
        HIPCHK(c, hipMemsetAsync(ctl + 4, 0, 2 * sizeof(uint32_t), c->stream));
        gr_prev_commit<<<blocks_for(n), 256, 0, c->stream>>>(n, fdist, out_prev, cand, ctl);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(c->u_host, ctl + 4, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ++waits;
        ++launches;
        if (pass > 0 && c->u_host[1] > 0u) ++rounds2;
        if (c->u_host[0] == 0u || (pass > 0 && c->u_host[1] == 0u)) break;  // none left, or a round that resolved none
        gr_prev_tier2<<<blocks_for(m), 256, 0, c->stream>>>(lines, weights, m, fdist, out_prev, cand);
        KCHK(c);
        ++launches;
    }
    gr_prev_finish<<<blocks_for(n), 256, 0, c->stream>>>(n, out_prev);
    KCHK(c);
    ++launches;
    if (info5) {
        info5[0] = 1;
        info5[1] = launches;
        info5[2] = waits;
        info5[3] = rounds;
        info5[4] = rounds2;
    }
    return MI_ICP_OK;
}

}  // extern "C"
