"""CPU restatements of PointCloud::ClusterDBSCAN (geometry/pointcloud_cluster.cu:109-179 of the reference; the contract
is stated in include/mi_icp.h): numpy + scipy.

  rows(pts, eps, max_edges)               -> CSR (indptr, idx): row(i) = the nearest max_edges + 1 points with fp32
                                             d2 < eps*eps (d2 formed as outlier_exact.d2_f32 forms it), sorted by
                                             (d2, index) -- every candidate within eps from a cKDTree pair search with
                                             a small margin
  literal(pts, eps, min_points, max_edges)       the reference line by line: degrees with the point itself dropped and
                                             non-core rows cleared, then the host loop over the points -- a BFS from
                                             every unvisited point, its reach relabelled (or set to -1), cluster += 1
  by_definition(pts, eps, min_points, max_edges) the root / largest-root form: strongly connected components
                                             (scipy.sparse.csgraph), their condensation walked in topological order
                                             for the smallest index and the largest root that reach each component
Both return (labels int32[n], degrees int32[n], n_clusters).

This is a helper module of the suite, not a conftest: tests import it by name."""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph
from scipy.spatial import cKDTree

import outlier_exact as ox

F32 = np.float32


def rows(pts, eps, max_edges):
    pts = np.ascontiguousarray(pts, F32)
    n = len(pts)
    K = int(max_edges) + 1
    r2 = F32(eps) * F32(eps)
    if n == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int64)
    tree = cKDTree(pts.astype(np.float64))
    pr = tree.query_pairs(float(eps) * (1.0 + 1e-5) + 1e-12, output_type="ndarray").astype(np.int64)
    d2 = ox.d2_f32(pts[pr[:, 0]], pts[pr[:, 1]]) if len(pr) else np.zeros(0, F32)
    pr, d2 = pr[d2 < r2], d2[d2 < r2]
    ii = np.arange(n, dtype=np.int64)
    src = np.concatenate([ii, pr[:, 0], pr[:, 1]])
    dst = np.concatenate([ii, pr[:, 1], pr[:, 0]])
    dd = np.concatenate([np.zeros(n, F32), d2, d2])        # (d2 is symmetric in fp32: the squares of -d and d)
    order = np.lexsort((dst, dd, src))
    src, dst = src[order], dst[order]
    start = np.searchsorted(src, ii)
    rank = np.arange(len(src)) - start[src]
    keep = rank < K
    src, dst = src[keep], dst[keep]
    indptr = np.searchsorted(src, np.arange(n + 1, dtype=np.int64))
    return indptr, dst


def neighbours(indptr, idx):
    """N(i) = row(i) without i, as CSR; deg(i) = |N(i)|"""
    n = len(indptr) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    keep = idx != src
    src, dst = src[keep], idx[keep]
    return np.searchsorted(src, np.arange(n + 1, dtype=np.int64)), dst, np.diff(
        np.searchsorted(src, np.arange(n + 1, dtype=np.int64))).astype(np.int32)


def edges(pts, eps, min_points, max_edges):
    """(src, dst, deg): the edges i -> j of every core i, and every point's degree"""
    ip, ix = rows(pts, eps, max_edges)
    nptr, nidx, deg = neighbours(ip, ix)
    n = len(deg)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(nptr))
    core = deg >= min_points
    keep = core[src]
    return src[keep], nidx[keep], deg


def asymmetric_edges(pts, eps, min_points, max_edges):
    """the number of edges i -> j (i core) with i not in N(j)"""
    src, dst, _ = edges(pts, eps, 0, max_edges)          # every N(i), core or not
    n = len(pts)
    have = set(zip(src.tolist(), dst.tolist()))
    ip, ix = rows(pts, eps, max_edges)
    _, _, deg = neighbours(ip, ix)
    core = deg >= min_points
    return sum(1 for a, b in have if core[a] and (b, a) not in have)


def literal(pts, eps, min_points, max_edges=100):
    ip, ix = rows(pts, eps, max_edges)
    n = len(ip) - 1
    # compute_vertex_degree_functor: the point itself dropped, the others counted; non-core rows cleared
    nbrs, deg = [], np.zeros(n, np.int32)
    for i in range(n):
        r = [int(j) for j in ix[ip[i]:ip[i + 1]] if j != i]
        deg[i] = len(r)
        nbrs.append(r if len(r) >= min_points else [])
    # the host loop (pointcloud_cluster.cu:147-178)
    cluster = 0
    visited = np.zeros(n, bool)
    clusters = np.full(n, -1, np.int32)
    for i in range(n):
        if visited[i]:
            continue
        xa = {i}
        fa = [i]
        while fa:                                           # bfs_functor, one level after the other
            nxt = []
            for v in fa:
                for j in nbrs[v]:
                    if j not in xa:
                        xa.add(j)
                        nxt.append(j)
            fa = nxt
        xs = np.fromiter(xa, np.int64, len(xa))
        is_noise = len(xs) < min_points
        clusters[xs] = -1 if is_noise else cluster
        visited[xs] = True
        if not is_noise:
            cluster += 1
    return clusters, deg, cluster


def by_definition(pts, eps, min_points, max_edges=100):
    src, dst, deg = edges(pts, eps, min_points, max_edges)
    n = len(deg)
    if n == 0:
        return np.zeros(0, np.int32), deg, 0
    A = sparse.csr_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(n, n))
    nc, comp = csgraph.connected_components(A, directed=True, connection="strong")
    cmin = np.full(nc, n, np.int64)
    np.minimum.at(cmin, comp, np.arange(n))
    # the condensation: its edges between components, walked level by level in topological order (Kahn)
    cs, cd = comp[src], comp[dst]
    off = cs != cd
    e = np.unique(np.stack([cs[off], cd[off]], 1), axis=0) if off.any() else np.zeros((0, 2), np.int64)
    indeg = np.bincount(e[:, 1], minlength=nc)
    out_ptr = np.searchsorted(e[:, 0], np.arange(nc + 1))
    levels = []
    level = np.flatnonzero(indeg == 0)
    while len(level):
        levels.append(level)
        sel = np.concatenate([np.arange(out_ptr[c], out_ptr[c + 1]) for c in level]) if len(level) else []
        sel = np.asarray(sel, np.int64)
        np.subtract.at(indeg, e[sel, 1], 1)
        nxt = np.unique(e[sel, 1])
        level = nxt[indeg[nxt] == 0]
    assert sum(len(lv) for lv in levels) == nc, "the condensation is not acyclic"

    def walk(val, op):
        for lv in levels:
            sel = np.concatenate([np.arange(out_ptr[c], out_ptr[c + 1]) for c in lv]).astype(np.int64)
            op.at(val, e[sel, 1], val[e[sel, 0]])
        return val
    m = walk(cmin.copy(), np.minimum)                     # the smallest index that reaches each component
    root = m == cmin                                      # its smallest member is a root
    M = walk(np.where(root, cmin, -1), np.maximum)        # the largest root that reaches it
    core = deg >= min_points
    start = np.zeros(n, bool)
    rc = cmin[root]
    start[rc] = core[rc] | (min_points <= 1)              # |reach| >= min_points: core roots, lone points if <= 1
    number = np.cumsum(start) - 1
    r = M[comp]
    labels = np.where(start[r], number[r], -1).astype(np.int32)
    return labels, deg, int(start.sum())
