"""geometry.Graph and its search without a GPU: the numpy restatement (tests/graph_exact.py) gives the reference's own
unit-test values, agrees with scipy's Dijkstra where every fp32 sum is exact, reaches the same bits in any relaxation
order, its closed-form lattice equals brute force; csrc/graph_rules.h equals it in a stand-alone sanitized program;
the ABI family is declared, exported and bound, and the statuses that need no device come back."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_exact as gx
from conftest import ROOT

F = np.float32


def test_restatement_gives_the_reference_unit_test_values():
    n, lines, w, start = gx.small_cases()["five"]
    assert len(lines) == 10
    assert gx.offsets_of(lines, n).tolist() == [0, 2, 4, 6, 9, 10]
    dist, prev = gx.sssp(lines, w, n, start)
    assert dist.tolist() == [0.0, 1.0, 2.0, 2.0, 3.0]
    assert prev.tolist() == [0, 0, 0, 1, 3]
    assert gx.path(dist, prev, 0, 4) == ([0, 1, 3, 4], 3.0)
    assert gx.path(dist, prev, 0, 0) == ([0], 0.0)


def test_small_cases_resolve_every_reachable_node_without_cycles():
    for name, (n, lines, w, start) in gx.small_cases().items():
        dist, prev = gx.sssp(lines, w, n, start)
        assert prev[start] == start, name
        for v in range(n):
            assert (prev[v] == -1) == (not np.isfinite(dist[v])), (name, v)
            if prev[v] >= 0:
                nodes, length = gx.path(dist, prev, start, v)       # (raises on a cycle)
                assert nodes[0] == start and nodes[-1] == v and length == dist[v], name
    n, lines, w, start = gx.small_cases()["zero_pair_trap"]
    dist, prev = gx.sssp(lines, w, n, start)
    assert dist.tolist() == [4.0, 1.0, 1.0, 0.0] and prev.tolist() == [3, 3, 1, 3]
    n, lines, w, start = gx.small_cases()["zero_chain"]
    dist = gx.distances(lines, w, n, start)
    assert gx.predecessors(lines, w, dist, start)[1] >= 4              # the chain needs its tier-2 rounds
    n, lines, w, start = gx.small_cases()["tiny_after_1000"]
    dist, prev = gx.sssp(lines, w, n, start)
    assert dist.tolist() == [0.0, 1000.0, 1000.0, 1001.0] and prev.tolist() == [0, 0, 1, 2]


def _random_graph(rng, n, m, directed):
    l = rng.integers(0, n, size=(m, 2)).astype(np.int32)
    w = rng.integers(0, 1000, size=m).astype(F)
    if not directed:
        l, w = np.concatenate([l, l[:, ::-1]]), np.concatenate([w, w])
    l, w, _, _ = gx.construct(l, n, w)
    return l, w


@pytest.mark.parametrize("directed", [True, False])
def test_against_scipy_dijkstra_where_every_sum_is_exact(directed):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    rng = np.random.default_rng(5 + int(directed))
    for trial in range(12):
        n = int(rng.integers(2, 301))
        l, w = _random_graph(rng, n, int(rng.integers(1, 4 * n)), directed)
        start = int(rng.integers(0, n))
        # scipy drops explicit zeros and sums duplicates: keep the least weight per (u, v), shifted by 1 to stay explicit
        key = l[:, 0].astype(np.int64) * n + l[:, 1]
        order = np.lexsort((w, key))
        first = np.concatenate([[True], key[order][1:] != key[order][:-1]])
        ul, uw = l[order][first], w[order][first]
        mat = sp.csr_matrix((uw.astype(np.float64) + 1.0, (ul[:, 0], ul[:, 1])), shape=(n, n))
        mat.data -= 1.0
        want = dijkstra(mat, directed=True, indices=start)
        dist, prev = gx.sssp(l, w, n, start)
        assert np.array_equal(dist.astype(np.float64), want)
        for v in range(n):
            if v == start or prev[v] < 0:
                continue
            tight = (l[:, 0] == prev[v]) & (l[:, 1] == v) & ((dist[prev[v]] + w).astype(F) == dist[v])
            assert tight.any()
            assert gx.path(dist, prev, start, v)[0][0] == start


def test_bellman_ford_in_any_edge_order_reaches_the_same_bits():
    rng = np.random.default_rng(11)
    pool = np.array([0.0, 1e-6, 1000.0, np.inf, 1.0, 0.25], F)
    for trial in range(25):
        n = int(rng.integers(2, 40))
        m = int(rng.integers(1, 5 * n))
        l = rng.integers(0, n, size=(m, 2)).astype(np.int32)
        w = pool[rng.integers(0, len(pool), size=m)]
        l, w, _, _ = gx.construct(l, n, w)
        start = int(rng.integers(0, n))
        want = gx.distances(l, w, n, start)
        for _ in range(3):
            got = gx.distances(l, w, n, start, order=rng.permutation(len(l)))
            assert got.tobytes() == want.tobytes()
        end = int(rng.integers(0, n))
        d_end, p_end = gx.sssp(l, w, n, start, end)
        d_all, p_all = gx.sssp(l, w, n, start)
        keep = d_all <= d_all[end] if np.isfinite(d_all[end]) else np.ones(n, bool)
        assert np.array_equal(d_end[keep], d_all[keep]) and np.array_equal(p_end[keep], p_all[keep])
        assert np.isinf(d_end[~keep]).all() and (p_end[~keep] == -1).all()


@pytest.mark.parametrize("res", [(1, 1, 1), (1, 1, 4), (2, 1, 3), (4, 3, 2), (3, 3, 3)])
def test_lattice_closed_form_equals_brute_force(res):
    brute = gx.lattice_edges_brute(res)
    lines = gx.lattice_edges(res)
    assert len(brute) == gx.lattice_edge_count(res)
    assert np.array_equal(lines, brute)
    rx, ry, rz = res
    off = gx.offsets_of(lines, rx * ry * rz)
    for x in range(rx):
        for y in range(ry):
            for z in range(rz):
                assert gx.lattice_edge_offset(x, y, z, res) == off[(x * ry + y) * rz + z]
    pts, _, w, _ = gx.lattice((-1, -2, 0.5), (1, 1, 2), res)
    assert pts.dtype == F and pts.shape == (rx * ry * rz, 3)
    assert np.array_equal(pts[0], np.array([-1, -2, 0.5], F))
    step = (np.array([1, 1, 2], F) - np.array([-1, -2, 0.5], F)) / np.array(res, F)
    assert np.array_equal(pts[-1], np.array([-1, -2, 0.5], F) + (np.array(res, F) - F(1)) * step)   # one step short of max
    assert (w > 0).all()


def test_header_rules_equal_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_graph_rules")
    src = os.path.join(ROOT, "tests", "cpp", "test_graph_rules.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cupoch_amd", "csrc"), src, "-o", exe])
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["graph_rules.h"]
    rng = np.random.default_rng(3)
    shapes = [(1, 1, 1), (1, 1, 4), (2, 1, 3), (4, 3, 2), (5, 1, 1), (3, 4, 5), (1, 7, 2)]
    text, want = [], []
    for res in shapes:
        rx, ry, rz = res
        text.append("L %d %d %d" % res)
        want.append([gx.lattice_edge_count(res)] + [gx.lattice_edge_offset(x, y, z, res)
                                                    for x in range(rx) for y in range(ry) for z in range(rz)])
    pool = np.array([0.0, 1e-6, 1.0, 1000.0, 1000.0000610351562, np.inf, 3.5, 2.5], F)
    tiers = []
    for _ in range(400):
        du, dv, w = pool[rng.integers(0, len(pool), 3)]
        with np.errstate(all="ignore"):
            s = F(du + w)
        text.append("T %08x %08x %08x" % tuple(int(np.array(v, F).view(np.uint32)) for v in (du, dv, w)))
        tiers.append([int(np.isfinite(dv) and du < dv and s == dv), int(np.isfinite(dv) and du == dv and s == dv)])
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [[int(t) for t in line.split()] for line in out if line.strip()]
    assert got[:len(want)] == want
    assert got[len(want):] == tiers
    assert any(t[0] for t in tiers) and any(t[1] for t in tiers)


GRAPH_NAMES = ["mi_icp_graph_construct", "mi_icp_graph_weights_from_distance", "mi_icp_graph_node_distances",
               "mi_icp_graph_lattice", "mi_icp_graph_set_edge_weights", "mi_icp_graph_remove_edges", "mi_icp_graph_sssp",
               "mi_icp_graph_sssp_limits"]


def test_abi_family_is_declared_exported_and_bound():
    from cupoch_amd import _lib
    src = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    for n in GRAPH_NAMES:
        assert re.search(r"MI_ICP_API\s+int\s+%s\s*\(" % n, src), n
        assert n in _lib.SIGNATURES
    assert "mi_graph" in _lib.UNITS
    assert os.path.exists(os.path.join(_lib.CSRC, "mi_graph.hip")) and os.path.exists(os.path.join(_lib.CSRC, "graph_kernels.h"))
    _lib.build()
    L = _lib.load()
    assert all(hasattr(L, n) for n in GRAPH_NAMES)
    for section in ("graph (geometry/graph", "Waits: construct once"):
        assert section in src


def test_statuses_that_need_no_device():
    from cupoch_amd import _lib
    from cupoch_amd.engine import Engine
    _lib.build()
    L = _lib.load()
    nmax, mmax, batch = Engine.graph_sssp_limits()
    assert nmax >= 1000 and mmax >= 26 * 1000 and batch >= 1       # the planner's own sizes are one launch
    n, m = C.c_int64(7), C.c_int64(7)
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    null = None
    # the lattice's counts are closed forms: no context, no device
    lat = lambda res, pc, ec: L.mi_icp_graph_lattice(null, lo, hi, (C.c_int32 * 3)(*res), null, pc, null, null, ec, null,
                                                     C.byref(n), C.byref(m))
    assert lat((4, 3, 2), 0, 0) == 0 and (n.value, m.value) == (24, gx.lattice_edge_count((4, 3, 2)))
    assert lat((1, 1, 1), 0, 0) == 0 and (n.value, m.value) == (1, 0)
    for res in ((0, 3, 2), (4, -1, 2), (4, 3, 0)):
        assert lat(res, 0, 0) == -1 and (n.value, m.value) == (0, 0)        # a resolution below 1
    assert lat((4, 3, 2), -1, 0) == -1 and lat((4, 3, 2), 0, -1) == -1      # a negative capacity
    assert lat((1291, 1291, 1291), 0, 0) == -1                              # more than 0x7fffff00 nodes
    assert lat((900, 900, 900), 0, 0) == -1                                 # more than 2^31 - 1 edges
    assert lat((4, 3, 2), 24, 256) == -1                                    # room to write, but no context
    # no context: refused before anything else
    assert L.mi_icp_graph_construct(null, null, null, null, 0, 0, null) == -1
    assert L.mi_icp_graph_sssp(null, null, null, null, 1, 0, 0, -1, null, null, null) == -1
    assert L.mi_icp_graph_remove_edges(null, null, null, null, -1, 0, null, 0, 0, null, C.byref(m)) == -1
    import torch
    if torch.cuda.is_available():
        pytest.skip("the context-level statuses are covered by tests/test_gpu_graph.py")
    ctx = C.c_void_p()
    assert L.mi_icp_create(0, C.byref(ctx)) == -5                   # MI_ICP_ERR_NO_DEVICE: no context to ask further


def test_python_surface_names_and_defaults():
    import inspect
    from cupoch_amd import geometry, planning
    G = geometry.Graph
    for name in ("edges", "edge_weights", "edge_index_offsets", "node_colors", "has_weights", "has_node_colors", "is_constructed",
                 "construct_graph", "connect_to_nearest_neighbors", "add_node_and_connect", "add_edge", "add_edges",
                 "remove_edge", "remove_edges", "set_edge_weights_from_distance", "set_edge_weights", "paint_edge_color",
                 "paint_edges_color", "paint_node_color", "paint_nodes_color", "dijkstra_paths", "dijkstra_path",
                 "create_from_axis_aligned_bounding_box"):
        assert hasattr(G, name), name
    assert issubclass(G, geometry.LineSet)
    sig = inspect.signature
    assert sig(G.construct_graph).parameters["set_edge_weights_from_distance"].default is True
    assert sig(G.connect_to_nearest_neighbors).parameters["max_num_edges"].default == 30
    assert sig(G.add_node_and_connect).parameters["max_edge_distance"].default == 0.0
    assert sig(G.add_node_and_connect).parameters["lazy_add"].default is False
    assert sig(G.add_edge).parameters["weight"].default == 1.0
    assert sig(G.dijkstra_paths).parameters["end_node_index"].default == -1
    p = sig(planning.Pos3DPlanner.__init__).parameters
    assert p["object_radius"].default == 0.1 and p["max_edge_distance"].default == 1.0
    for name in ("add_obstacle", "update_graph", "find_path", "get_graph"):
        assert hasattr(planning.Pos3DPlanner, name)
