// graph_rules.h -- the rules of geometry::Graph<3> that host and device share (include/mi_icp.h "graph"): the lattice's
// index arithmetic with its closed-form edge offsets, and the two predecessor predicates of the search.  Plain C++: the
// kernels (graph_kernels.h), the launcher (mi_graph.hip) and a stand-alone host program include it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MI_GRAPH_HD __host__ __device__ inline
#else
#define MI_GRAPH_HD inline
#endif

namespace mi {
namespace graph {

constexpr uint32_t kInfBits = 0x7f800000u;  // +inf: the largest pattern a distance takes (non-negative floats order as their bits)
constexpr int32_t kUnresolved = 0x7fffffff; // a predecessor not found yet: above every node index, so atomicMin replaces it

// c(t): how many of t - 1, t, t + 1 lie in [0, r)
MI_GRAPH_HD int64_t lattice_axis_count(int64_t t, int64_t r) { return 1 + (t > 0 ? 1 : 0) + (t < r - 1 ? 1 : 0); }
// c(0) + ... + c(k - 1), 0 <= k <= r
MI_GRAPH_HD int64_t lattice_axis_prefix(int64_t k, int64_t r) {
    const int64_t a = k > 1 ? k - 1 : 0, b = k < r - 1 ? k : r - 1;
    return k + a + (k > 0 ? b : 0);
}
// every ordered pair of lattice nodes that are neighbours (26-connected), i != j
MI_GRAPH_HD int64_t lattice_edge_count(int64_t rx, int64_t ry, int64_t rz) {
    return (3 * rx - 2) * (3 * ry - 2) * (3 * rz - 2) - rx * ry * rz;
}
// the first edge of node (x, y, z) = (x*ry + y)*rz + z when the edges ascend in (i, j): the neighbour counts, self
// included, of every node before it, minus those nodes
MI_GRAPH_HD int64_t lattice_edge_offset(int64_t x, int64_t y, int64_t z, int64_t rx, int64_t ry, int64_t rz) {
    const int64_t sy = 3 * ry - 2, sz = 3 * rz - 2;
    const int64_t before = lattice_axis_prefix(x, rx) * sy * sz +
                           lattice_axis_count(x, rx) * (lattice_axis_prefix(y, ry) * sz + lattice_axis_count(y, ry) * lattice_axis_prefix(z, rz));
    return before - ((x * ry + y) * rz + z);
}

// tier 1: u is a predecessor of v that lies strictly nearer.  du, dv: distances, w the edge's weight; sum = (float)(du + w)
MI_GRAPH_HD bool tier1_ok(float du, float dv, float sum) { return dv < __builtin_inff() && du < dv && sum == dv; }
// tier 2: u (resolved) and v (not) at one distance, joined by an edge that adds nothing in fp32
MI_GRAPH_HD bool tier2_ok(float du, float dv, float sum) { return dv < __builtin_inff() && du == dv && sum == dv; }

}  // namespace graph
}  // namespace mi
