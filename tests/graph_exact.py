"""The contract of include/mi_icp.h ("graph") and of planning.Pos3DPlanner.find_path, restated in numpy: what the GPU
tests hold the library to, bit for bit.  fp32 throughout, in the order the header writes; nothing here is fast."""
import numpy as np

import collision_exact as cx

F = np.float32
INF = F(np.inf)
UNRES = np.iinfo(np.int32).max


# ---------------------------------------------------------------------------------------------- construct
def offsets_of(lines, n_points):
    first = np.asarray(lines, np.int64).reshape(-1, 2)[:, 0]
    return np.searchsorted(first, np.arange(n_points + 1), side="left").astype(np.int32)


def construct(lines, n_points, weights=None, colors=None):
    """-> (lines, weights, colors, offsets): a stable sort by (first, second)"""
    lines = np.asarray(lines, np.int32).reshape(-1, 2)
    if len(lines) and (lines.min() < 0 or lines.max() >= n_points):
        raise ValueError("a line's point index is out of range")
    order = np.lexsort((lines[:, 1], lines[:, 0]))          # (lexsort is stable)
    lines = lines[order]
    w = None if weights is None else np.asarray(weights, F)[order]
    c = None if colors is None else np.asarray(colors, F).reshape(-1, 3)[order]
    return lines, w, c, offsets_of(lines, n_points)


def distance(a, b):
    """sqrtf((dx*dx + dy*dy) + dz*dz), d = a - b"""
    d = np.asarray(a, F) - np.asarray(b, F)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(F)


def weights_from_distance(points, lines):
    points, lines = np.asarray(points, F).reshape(-1, 3), np.asarray(lines, np.int64).reshape(-1, 2)
    return distance(points[lines[:, 0]], points[lines[:, 1]])


# ---------------------------------------------------------------------------------------------- lattice
def lattice_points(mn, mx, res):
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    rx, ry, rz = [int(r) for r in res]
    steps = (mx - mn) / np.asarray(res, np.int32).astype(F)
    x, y, z = np.meshgrid(np.arange(rx), np.arange(ry), np.arange(rz), indexing="ij")
    g = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F)
    return (mn[None, :] + g * steps[None, :]).astype(F)


def lattice_edges_brute(res):
    """every ordered pair of 26-neighbours, found node by node and sorted"""
    rx, ry, rz = [int(r) for r in res]
    out = []
    for x in range(rx):
        for y in range(ry):
            for z in range(rz):
                i = (x * ry + y) * rz + z
                for dx in (1, -1, 0):
                    for dy in (0, 1, -1):
                        for dz in (-1, 1, 0):
                            nx, ny, nz = x + dx, y + dy, z + dz
                            if (dx, dy, dz) != (0, 0, 0) and 0 <= nx < rx and 0 <= ny < ry and 0 <= nz < rz:
                                out.append((i, (nx * ry + ny) * rz + nz))
    return np.array(sorted(out), np.int32).reshape(-1, 2)


def lattice_edge_count(res):
    rx, ry, rz = [int(r) for r in res]
    return (3 * rx - 2) * (3 * ry - 2) * (3 * rz - 2) - rx * ry * rz


def _axis_count(t, r):
    return 1 + (t > 0) + (t < r - 1)


def _axis_prefix(k, r):
    return k + max(k - 1, 0) + min(k, r - 1)


def lattice_edge_offset(x, y, z, res):
    """the closed form of csrc/graph_rules.h"""
    rx, ry, rz = [int(r) for r in res]
    sy, sz = 3 * ry - 2, 3 * rz - 2
    before = _axis_prefix(x, rx) * sy * sz + _axis_count(x, rx) * (_axis_prefix(y, ry) * sz + _axis_count(y, ry) * _axis_prefix(z, rz))
    return before - ((x * ry + y) * rz + z)


def lattice_edges(res):
    """the edges in ascending (i, j) order by the closed form: node by node, neighbours by ascending offset"""
    rx, ry, rz = [int(r) for r in res]
    n = rx * ry * rz
    i = np.arange(n, dtype=np.int64)
    x, y, z = i // (ry * rz), (i % (ry * rz)) // rz, i % rz
    cols = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) == (0, 0, 0):
                    continue
                nx, ny, nz = x + dx, y + dy, z + dz
                ok = (nx >= 0) & (nx < rx) & (ny >= 0) & (ny < ry) & (nz >= 0) & (nz < rz)
                cols.append(np.where(ok, (nx * ry + ny) * rz + nz, -1))
    j = np.stack(cols, axis=1)                      # [n, 26], ascending along a row where valid
    keep = j >= 0
    lines = np.stack([np.repeat(i[:, None], 26, axis=1)[keep], j[keep]], axis=1).astype(np.int32)
    return lines


def lattice(mn, mx, res):
    """-> (points, lines, weights, offsets)"""
    if min(int(r) for r in res) < 1:
        raise ValueError("a resolution below 1")
    pts = lattice_points(mn, mx, res)
    lines = lattice_edges(res)
    return pts, lines, weights_from_distance(pts, lines), offsets_of(lines, len(pts))


# ---------------------------------------------------------------------------------------------- edge updates
def match(lines, edges, is_directed):
    """bool[m]: the lines equal to a listed edge (or, undirected, to the reverse of one)"""
    lines = np.asarray(lines, np.int64).reshape(-1, 2)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    if not is_directed:
        edges = np.concatenate([edges, edges[:, ::-1]])
    big = np.int64(1) << 32
    return np.isin(lines[:, 0] * big + lines[:, 1], edges[:, 0] * big + edges[:, 1])


def set_edge_weights(lines, weights, edges, weight, is_directed):
    w = np.asarray(weights, F).copy()
    w[match(lines, edges, is_directed)] = F(weight)
    return w


def remove_edges(lines, n_points, edges, is_directed, weights=None, colors=None):
    keep = ~match(lines, edges, is_directed)
    lines = np.asarray(lines, np.int32).reshape(-1, 2)[keep]
    return (lines, None if weights is None else np.asarray(weights, F)[keep],
            None if colors is None else np.asarray(colors, F).reshape(-1, 3)[keep], offsets_of(lines, n_points))


def connect_to_nearest_neighbors(points, lines, weights, max_edge_distance, max_num_edges, is_directed):
    """-> (lines, weights, offsets).  Per query i the max_num_edges + 1 nearest points with d2 < r^2 (ties by index);
    i itself dropped; the reverse added when undirected; edges already there not added; weights by distance."""
    pts = np.asarray(points, F).reshape(-1, 3)
    n = len(pts)
    d = pts[:, None, :].astype(np.float64) - pts[None, :, :].astype(np.float64)
    d2 = (d * d).sum(axis=2)
    new = set()
    for i in range(n):
        order = np.lexsort((np.arange(n), d2[i]))
        order = [j for j in order if d2[i, j] < float(F(max_edge_distance)) ** 2][:max_num_edges + 1]
        for j in order:
            if j != i:
                new.add((i, int(j)))
                if not is_directed:
                    new.add((int(j), i))
    have = set(map(tuple, np.asarray(lines, np.int64).reshape(-1, 2).tolist()))
    add = np.array(sorted(new - have), np.int32).reshape(-1, 2)
    all_lines = np.concatenate([np.asarray(lines, np.int32).reshape(-1, 2), add])
    all_w = np.concatenate([np.asarray(weights, F).reshape(-1), weights_from_distance(pts, add)])
    out_lines, out_w, _, off = construct(all_lines, n, all_w)
    return out_lines, out_w, off


def add_node_and_connect(points, lines, weights, point, max_edge_distance, is_directed):
    """-> (points, lines, weights) NOT constructed: edges (i, n) for d < max_edge_distance, then the reverses"""
    pts = np.asarray(points, F).reshape(-1, 3)
    n = len(pts)
    q = np.asarray(point, F).reshape(3)
    d = distance(pts, q[None, :])
    near = np.flatnonzero(d < F(max_edge_distance)).astype(np.int32)
    fwd = np.stack([near, np.full(len(near), n, np.int32)], axis=1)
    new_l, new_w = (fwd, d[near]) if is_directed else (np.concatenate([fwd, fwd[:, ::-1]]), np.concatenate([d[near], d[near]]))
    return (np.concatenate([pts, q[None, :]]), np.concatenate([np.asarray(lines, np.int32).reshape(-1, 2), new_l.astype(np.int32)]),
            np.concatenate([np.asarray(weights, F).reshape(-1), new_w.astype(F)]))


# ---------------------------------------------------------------------------------------------- the search
def distances(lines, weights, n, start, order=None):
    """Bellman-Ford from +inf, all edges per round (or one by one in `order`), until nothing changes"""
    lines = np.asarray(lines, np.int64).reshape(-1, 2)
    w = np.asarray(weights, F).reshape(-1)
    if len(w) and not (w >= 0).all():
        raise ValueError("a weight is negative or NaN")
    dist = np.full(n, INF, F)
    dist[start] = F(0)
    u, v = lines[:, 0], lines[:, 1]
    with np.errstate(all="ignore"):
        while True:
            if order is None:
                new = dist.copy()
                np.minimum.at(new, v, (dist[u] + w).astype(F))
            else:
                new = dist.copy()
                for e in order:
                    s = F(new[u[e]] + w[e])
                    if s < new[v[e]]:
                        new[v[e]] = s
            if np.array_equal(new, dist):
                return dist
            dist = new


def predecessors(lines, weights, dist, start):
    """the two tiers; -> (prev int32[n], the number of tier-2 rounds that resolved a node)"""
    lines = np.asarray(lines, np.int64).reshape(-1, 2)
    w = np.asarray(weights, F).reshape(-1)
    u, v = lines[:, 0], lines[:, 1]
    n = len(dist)
    prev = np.full(n, UNRES, np.int64)
    prev[start] = start
    with np.errstate(all="ignore"):
        s = (dist[u] + w).astype(F)
    du, dv = dist[u], dist[v]
    t1 = np.isfinite(dv) & (du < dv) & (s == dv) & (v != start)
    np.minimum.at(prev, v[t1], u[t1])
    rounds = 0
    while True:
        t2 = np.isfinite(dv) & (prev[v] == UNRES) & (prev[u] != UNRES) & (du == dv) & (s == dv)
        if not t2.any():
            break
        cand = np.full(n, UNRES, np.int64)
        np.minimum.at(cand, v[t2], u[t2])
        prev = np.where(cand != UNRES, cand, prev)
        rounds += 1
    prev[prev == UNRES] = -1
    return prev.astype(np.int32), rounds


def sssp(lines, weights, n, start, end=-1):
    """-> (dist float32[n], prev int32[n])"""
    dist = distances(lines, weights, n, start)
    if end >= 0 and np.isfinite(dist[end]):
        dist = np.where(dist > dist[end], INF, dist).astype(F)
    prev, _ = predecessors(lines, weights, dist, start)
    return dist, prev


def path(dist, prev, start, end):
    """-> (nodes, length): ([], inf) when the end is unreachable, ([start], 0.0) for start == end"""
    if prev[end] < 0:
        return [], float("inf")
    nodes = [int(end)]
    while nodes[-1] != start:
        nodes.append(int(prev[nodes[-1]]))
        if len(nodes) > len(prev):
            raise RuntimeError("the predecessors cycle")
    return nodes[::-1], float(dist[end])


# ---------------------------------------------------------------------------------------------- the planner
def find_path(points, lines, start, goal, obstacles, object_radius, max_edge_distance, is_directed=False):
    """Pos3DPlanner.find_path: copy, add the start lazily and the goal, weights from distance, colliding lines at
    +inf, search n -> n + 1.  obstacles: sides of collision_exact (("voxel", keys, vs, origin) / ("occ", idx, res, vs,
    origin)).  -> (path points float32[k, 3], lines, weights)"""
    n = len(points)
    w0 = np.zeros(len(lines), F)
    pts, ls, ws = add_node_and_connect(points, lines, w0, start, max_edge_distance, is_directed)
    pts, ls, ws = add_node_and_connect(pts, ls, ws, goal, max_edge_distance, is_directed)
    ls, _, _, _ = construct(ls, n + 2, ws)
    ws = weights_from_distance(pts, ls)
    for side in obstacles:
        pairs = cx.compute_intersection(side, ("lines", pts, ls), object_radius)
        ws = set_edge_weights(ls, ws, ls[pairs[:, 1]], INF, is_directed)
    dist, prev = sssp(ls, ws, n + 2, n, n + 1)
    nodes, _ = path(dist, prev, n, n + 1)
    return pts[nodes].reshape(-1, 3).astype(F), ls, ws


# ---------------------------------------------------------------------------------------------- shared small cases
def _undirected(edges):
    out = []
    for a, b, w in edges:
        out += [(a, b, w), (b, a, w)]
    return out


def small_cases():
    """name -> (n, lines int32 [m, 2] constructed, weights float32 [m], start): the smallest graphs on which each rule
    of the search can go wrong"""
    inf = float("inf")
    raw = {
        # src/tests/geometry/graph.cpp: offsets 0 2 4 6 9 10, distances 1 2 2 3
        "five": (5, _undirected([(0, 1, 1), (0, 2, 2), (1, 3, 1), (2, 3, 1), (3, 4, 1)]), 0),
        "directed": (5, [(0, 1, 1), (1, 2, 1), (2, 0, 1), (0, 3, 5), (3, 4, 1), (4, 1, 0.5), (2, 3, 1)], 0),
        "duplicates": (3, [(0, 1, 3), (0, 1, 1), (0, 1, 2), (1, 2, 1), (1, 2, 1), (1, 0, 7)], 0),
        "lonely_start": (4, _undirected([(0, 1, 1), (1, 2, 1)]), 3),
        "two_components": (6, _undirected([(0, 1, 1), (1, 2, 2), (3, 4, 1), (4, 5, 1)]), 1),
        # a = 1 and b = 2 joined by weight 0, a entered from node 3: "smallest tight predecessor" makes them name each other
        "zero_pair_trap": (4, _undirected([(1, 2, 0)]) + [(3, 1, 1), (3, 0, 4)], 3),
        # 1e-6 is below half an ulp of 1000: the edge adds nothing
        "tiny_after_1000": (4, [(0, 1, 1000), (1, 2, 1e-6), (2, 3, 1)], 0),
        "zero_chain": (8, [(0, 1, 1)] + _undirected([(i, i + 1, 0) for i in range(1, 6)]) + [(6, 7, 2)], 0),
        "inf_edges": (5, _undirected([(0, 1, 1), (1, 2, inf), (0, 3, 4), (3, 2, 1), (2, 4, inf)]), 0),
        "plateau": (7, _undirected([(0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 4, 1), (2, 4, 1), (3, 5, 1), (5, 6, 3)]), 0),
    }
    out = {}
    for name, (n, edges, start) in raw.items():
        l = np.array([(a, b) for a, b, _ in edges], np.int32).reshape(-1, 2)
        w = np.array([w for _, _, w in edges], F)
        l, w, _, _ = construct(l, n, w)
        out[name] = (n, l, w, start)
    return out
