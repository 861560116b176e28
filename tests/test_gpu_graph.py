"""geometry.Graph on the GPU, through the Python mirror and the C ABI, against the numpy restatement of the contract
(tests/graph_exact.py): distances equal bit for bit, predecessors exactly, always -- in every launcher regime, entered
at the smallest n and m that select it and one below, with the boundary read from the library; twice, with identical
bytes.  Then construct, the edge updates, the neighbour connections, the strictness of add_node_and_connect, the
lattice."""
import time

import numpy as np
import pytest

import graph_exact as gx

pytestmark = pytest.mark.gpu
F = np.float32
INF = float("inf")


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd import geometry
    return geometry.get_engine()


@pytest.fixture(scope="module")
def limits():
    from cupoch_amd.engine import Engine
    return Engine.graph_sssp_limits()


def dev(eng, a, dtype, cols):
    return eng._vg_dev(np.ascontiguousarray(a, dtype), dtype, cols)


def abi_sssp(eng, n, lines, w, start, end=-1):
    """the raw entry point on a constructed edge list -> (dist, prev, info)"""
    off = dev(eng, gx.offsets_of(lines, n), np.int32, 1)
    d, p, info = eng.graph_sssp(off, dev(eng, lines, np.int32, 2), dev(eng, w, F, 1), n, start, end, want_info=True)
    return to_np(d), to_np(p), info


def graph_of(n, lines, w, directed=True):
    from cupoch_amd import geometry
    g = geometry.Graph(np.zeros((n, 3), F))
    g.is_directed = directed
    g.lines = np.ascontiguousarray(lines, np.int32)
    g.edge_weights = np.ascontiguousarray(w, F)
    return g.construct_graph(False)


def check_sssp(eng, n, lines, w, start, end=-1, regime=None, want=None):
    """both surfaces, twice each: bits of dist, prev exactly; -> info of the ABI call"""
    want_d, want_p = want if want is not None else gx.sssp(lines, w, n, start, end)
    outs = []
    for _ in range(2):
        d, p, info = abi_sssp(eng, n, lines, w, start, end)
        outs.append((d.tobytes(), p.tobytes()))
        assert d.tobytes() == want_d.tobytes() and np.array_equal(p, want_p)
        if regime is not None:
            assert info[0] == regime
    assert outs[0] == outs[1]
    g = graph_of(n, lines, w)
    assert np.array_equal(to_np(g.edges.tensor), lines) and g.is_constructed()      # (already sorted: construct keeps it)
    d, p = g.dijkstra_paths(start, end)
    assert to_np(d).tobytes() == want_d.tobytes() and np.array_equal(to_np(p), want_p)
    return info


def padded(want, n_to):
    d, p = want
    k = n_to - len(d)
    return np.concatenate([d, np.full(k, np.inf, F)]), np.concatenate([p, np.full(k, -1, np.int32)])


# ------------------------------------------------------------------------------------------------ the search
@pytest.mark.parametrize("name", sorted(gx.small_cases()))
def test_small_cases_in_both_regimes(eng, limits, name):
    n, lines, w, start = gx.small_cases()[name]
    want = gx.sssp(lines, w, n, start)
    info = check_sssp(eng, n, lines, w, start, regime=0, want=want)
    assert info[1] == 1 and info[2] == 1                      # the small regime: one launch, one wait
    big = limits[0] + 1                                       # the same graph beside isolated nodes: the large regime
    info = check_sssp(eng, big, lines, w, start, regime=1, want=padded(want, big))
    if name == "zero_chain":
        assert info[4] >= 4                                   # the tier-2 rounds ran
    if name == "five":
        from cupoch_amd import geometry
        g = geometry.Graph(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 2, 0]], F))
        for e, wt in (((0, 1), 1.0), ((0, 2), 2.0), ((1, 3), 1.0), ((2, 3), 1.0), ((3, 4), 1.0)):
            g.add_edge(e, wt)
        assert len(g.lines) == 10 and to_np(g.edge_index_offsets).tolist() == [0, 2, 4, 6, 9, 10]
        d, p = g.dijkstra_paths(0)
        assert to_np(d).tolist() == [0.0, 1.0, 2.0, 2.0, 3.0]
        assert g.dijkstra_path(0, 4) == ([0, 1, 3, 4], 3.0)
        assert g.dijkstra_path(2, 2) == ([2], 0.0)
    if name == "two_components":
        g = graph_of(n, lines, w)
        assert g.dijkstra_path(1, 4) == ([], INF)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), -1e-30])
def test_bad_weights_are_refused_in_both_regimes(eng, limits, bad):
    from cupoch_amd import MiIcpError
    n, lines, w, start = gx.small_cases()["five"]
    w = w.copy()
    w[3] = bad
    for nn in (n, limits[0] + 1):
        with pytest.raises(MiIcpError) as e:
            abi_sssp(eng, nn, lines, w, start)
        assert e.value.code == -1 and "weight" in str(e.value)
    w[3] = -0.0                                               # minus zero is a zero
    assert abi_sssp(eng, n, lines, w, start)[0].tobytes() == gx.sssp(lines, w, n, start)[0].tobytes()


def test_bad_graphs_are_refused(eng, limits):
    from cupoch_amd import MiIcpError
    n, lines, w, start = gx.small_cases()["five"]
    for nn in (n, limits[0] + 1):
        bad = lines.copy()
        bad[4, 1] = nn
        with pytest.raises(MiIcpError):
            abi_sssp(eng, nn, bad, w, start)
    off = gx.offsets_of(lines, limits[0] + 1)
    off[3] = len(lines) + 5                                   # the large regime walks the offsets: checked first
    with pytest.raises(MiIcpError):
        eng.graph_sssp(dev(eng, off, np.int32, 1), dev(eng, lines, np.int32, 2), dev(eng, w, F, 1), limits[0] + 1, 0)
    for s, e in ((-1, -1), (n, -1), (0, n)):
        with pytest.raises(MiIcpError):
            abi_sssp(eng, n, lines, w, s, e)


@pytest.mark.parametrize("big", [False, True])
def test_early_end(eng, limits, big):
    cases = gx.small_cases()
    for name, ends in (("plateau", (4, 1, 6, 0)), ("two_components", (2, 4, 1)), ("zero_chain", (3, 7)), ("inf_edges", (2, 4))):
        n, lines, w, start = cases[name]
        full = gx.sssp(lines, w, n, start)
        nn = limits[0] + 1 if big else n
        for end in ends:
            want = gx.sssp(lines, w, n, start, end)
            keep = full[0] <= full[0][end] if np.isfinite(full[0][end]) else np.ones(n, bool)
            assert np.array_equal(want[0][keep], full[0][keep]) and np.array_equal(want[1][keep], full[1][keep])
            assert np.isinf(want[0][~keep]).all() and (want[1][~keep] == -1).all()
            check_sssp(eng, nn, lines, w, start, end, regime=int(big), want=padded(want, nn))


@pytest.fixture(scope="module")
def long_path():
    """3000 nodes in a row (weights that do not sum exactly), both directions"""
    n = 3000
    a = np.arange(n - 1, dtype=np.int32)
    w1 = (F(0.1) + (a % 7).astype(F) * F(0.013)).astype(F)
    lines, w, _, _ = gx.construct(np.concatenate([np.stack([a, a + 1], 1), np.stack([a + 1, a], 1)]), n, np.concatenate([w1, w1]))
    dist = np.zeros(n, F)
    for i in range(1, n):
        dist[i] = F(dist[i - 1] + w1[i - 1])                  # (the only path: the restatement's fixed point, in closed form)
    prev = np.concatenate([[0], np.arange(n - 1)]).astype(np.int32)
    return n, lines, w, (dist, prev)


@pytest.mark.parametrize("big", [False, True])
def test_path_of_3000_nodes_runs_many_rounds_quickly(eng, limits, long_path, big):
    n, lines, w, want = long_path
    nn = limits[0] + 1 if big else n
    abi_sssp(eng, nn, lines, w, 0)                            # (the first call allocates)
    t0 = time.perf_counter()
    d, p, info = abi_sssp(eng, nn, lines, w, 0)
    elapsed = time.perf_counter() - t0
    want = padded(want, nn)
    assert d.tobytes() == want[0].tobytes() and np.array_equal(p, want[1])
    assert info[0] == int(big) and info[3] >= n - 1
    if big:
        assert info[2] >= (n - 1) // limits[2]                # one wait per batch
    assert elapsed < 5.0, elapsed
    d, p, _ = abi_sssp(eng, nn, lines, w, 0, end=10)
    assert np.array_equal(d[:11], want[0][:11]) and np.isinf(d[11:]).all() and (p[11:] == -1).all()


@pytest.mark.parametrize("res", [(4, 3, 2), (12, 9, 7)])
def test_lattices_with_a_third_of_the_edges_removed(eng, limits, res):
    rng = np.random.default_rng(res[0])
    pts, lines, w, _ = gx.lattice((-1, -1, -1), (1, 2, 1.5), res)
    n = len(pts)
    w = w.copy()
    w[rng.random(len(w)) < 1 / 3] = np.inf
    want = gx.sssp(lines, w, n, 0)
    check_sssp(eng, n, lines, w, 0, regime=0, want=want)
    check_sssp(eng, limits[0] + 1, lines, w, 0, regime=1, want=padded(want, limits[0] + 1))
    end = n - 1
    want = gx.sssp(lines, w, n, 0, end)
    check_sssp(eng, n, lines, w, 0, end, regime=0, want=want)
    check_sssp(eng, limits[0] + 1, lines, w, 0, end, regime=1, want=padded(want, limits[0] + 1))


def _random_graph(rng, n, m):
    l = rng.integers(0, n, size=(m, 2)).astype(np.int32)
    w = rng.integers(0, 1000, size=m).astype(F) * F(0.37)
    w[rng.random(m) < 0.05] = 0
    l, w, _, _ = gx.construct(l, n, w)
    return l, w


@pytest.mark.parametrize("which", ["n_at", "n_above", "m_at", "m_above"])
def test_every_regime_at_its_boundary(eng, limits, which):
    nmax, mmax, _ = limits
    rng = np.random.default_rng({"n_at": 1, "n_above": 2, "m_at": 3, "m_above": 4}[which])
    if which.startswith("n"):
        n = nmax if which == "n_at" else nmax + 1
        m = 3 * n
    else:
        n = 2000
        m = mmax if which == "m_at" else mmax + 1
    lines, w = _random_graph(rng, n, m)
    lines[0] = (n - 1, 0)                                    # (the last node has an edge: the offsets' last entries count)
    lines, w, _, _ = gx.construct(lines, n, w)
    assert len(lines) == m
    start = int(lines[0, 0])
    info = check_sssp(eng, n, lines, w, start, regime=0 if which.endswith("at") else 1)
    assert (info[1] == 1) == which.endswith("at")


# ------------------------------------------------------------------------------------------------ construct and the updates
@pytest.mark.parametrize("n,m", [(7, 40), (300, 5000), (5000, 70000)])
def test_construct_is_stable_and_carries_weights_and_colours(eng, n, m):
    rng = np.random.default_rng(n)
    lines = rng.integers(0, n, size=(m, 2)).astype(np.int32)
    lines[m // 2:] = lines[:m - m // 2]                       # duplicates
    w = np.arange(m, dtype=F)                                 # (names every line: stability shows)
    col = rng.random((m, 3)).astype(F)
    wl, ww, wc, wo = gx.construct(lines, n, w, col)
    dl, dw, dc = dev(eng, lines, np.int32, 2), dev(eng, w, F, 1), dev(eng, col, F, 3)
    off = eng.graph_construct(dl, n, dw, dc)
    assert np.array_equal(to_np(dl), wl) and np.array_equal(to_np(dw), ww) and np.array_equal(to_np(dc), wc)
    assert np.array_equal(to_np(off), wo)
    dl = dev(eng, lines, np.int32, 2)
    assert np.array_equal(to_np(eng.graph_construct(dl, n)), wo) and np.array_equal(to_np(dl), wl)   # no weights, no colours
    from cupoch_amd import MiIcpError
    for bad in (-1, n):
        broken = lines.copy()
        broken[m // 3, 1] = bad
        dl, dw = dev(eng, broken, np.int32, 2), dev(eng, w, F, 1)
        with pytest.raises(MiIcpError) as e:
            eng.graph_construct(dl, n, dw)
        assert e.value.code == -1
        assert np.array_equal(to_np(dl), broken) and np.array_equal(to_np(dw), w)     # nothing written


@pytest.mark.parametrize("directed", [True, False])
def test_set_edge_weights_and_remove_edges(eng, directed):
    from cupoch_amd import geometry
    rng = np.random.default_rng(8 + int(directed))
    n, m = 60, 900
    lines = rng.integers(0, n, size=(m, 2)).astype(np.int32)
    w = rng.random(m).astype(F)
    col = rng.random((m, 3)).astype(F)
    listed = np.concatenate([lines[rng.integers(0, m, 40)], lines[rng.integers(0, m, 20)][:, ::-1], [[n - 1, n - 1], [0, 0], [500, 3]]]).astype(np.int32)
    g = geometry.Graph(rng.random((n, 3)).astype(F))
    g.is_directed = directed
    g.lines, g.edge_weights, g.colors = lines, w, col
    g.construct_graph(False)
    wl, ww, wc, wo = gx.construct(lines, n, w, col)
    assert np.array_equal(to_np(g.edges.tensor), wl) and np.array_equal(to_np(g.colors.tensor), wc)
    g.set_edge_weights(listed, INF)
    ww = gx.set_edge_weights(wl, ww, listed, INF, directed)
    assert np.array_equal(to_np(g.edge_weights), ww) and np.isinf(ww).sum() >= 40
    g.set_edge_weights(listed[:5], 2.5)
    ww = gx.set_edge_weights(wl, ww, listed[:5], 2.5, directed)
    assert np.array_equal(to_np(g.edge_weights), ww)
    g.remove_edges(listed[10:])
    rl, rw, rc, ro = gx.remove_edges(wl, n, listed[10:], directed, ww, wc)
    assert len(rl) < m
    assert np.array_equal(to_np(g.edges.tensor), rl) and np.array_equal(to_np(g.edge_weights), rw)
    assert np.array_equal(to_np(g.colors.tensor), rc) and np.array_equal(to_np(g.edge_index_offsets), ro)
    g.remove_edge(rl[0])
    rl2 = gx.remove_edges(rl, n, rl[:1], directed)[0]
    assert np.array_equal(to_np(g.edges.tensor), rl2) and g.is_constructed()
    g.set_edge_weights_from_distance()
    assert np.array_equal(to_np(g.edge_weights), gx.weights_from_distance(to_np(g.points.tensor), rl2))
    g.paint_edges_color(rl2[:3], (1, 0, 0))
    assert (to_np(g.colors.tensor)[gx.match(rl2, rl2[:3], directed)] == np.array([1, 0, 0], F)).all()
    g.paint_nodes_color([2, 5], (0, 1, 0))
    nc = to_np(g.node_colors.tensor)
    assert (nc[[2, 5]] == np.array([0, 1, 0], F)).all() and (np.delete(nc, [2, 5], 0) == 1).all()


def test_add_edges_without_weights_gives_one(eng):
    from cupoch_amd import geometry
    g = geometry.Graph(np.zeros((4, 3), F))
    g.add_edges(np.array([[0, 1], [1, 2]], np.int32))
    g.add_edges(np.array([[2, 3]], np.int32), np.array([4.0], F))
    assert to_np(g.edges.tensor).tolist() == [[0, 1], [1, 0], [1, 2], [2, 1], [2, 3], [3, 2]]
    assert to_np(g.edge_weights).tolist() == [1, 1, 1, 1, 4, 4]
    assert to_np(g.dijkstra_paths(0)[0]).tolist() == [0, 1, 2, 6]


@pytest.mark.parametrize("directed", [True, False])
def test_connect_to_nearest_neighbors(eng, directed):
    from cupoch_amd import geometry
    rng = np.random.default_rng(21)
    pts = rng.random((200, 3)).astype(F)
    radius, k = 0.25, 3
    d = np.linalg.norm(pts[:, None].astype(np.float64) - pts[None].astype(np.float64), axis=2)
    assert (np.abs(d - radius) > 1e-5).all()                          # no pair the radius could decide either way
    srt = np.sort(d, axis=1)
    assert (np.diff(srt[:, :k + 3], axis=1) > 1e-6).all()             # ... and no tie among the nearest
    assert ((d < radius).sum(axis=1) > k + 1).any()                   # lists are truncated
    first = np.array([[0, 1], [5, 7]], np.int32)
    g = geometry.Graph(pts)
    g.is_directed = directed
    g.add_edges(first, np.array([9.0, 8.0], F))
    have_l, have_w = to_np(g.edges.tensor).copy(), to_np(g.edge_weights).copy()
    g.connect_to_nearest_neighbors(radius, k)
    wl, ww, wo = gx.connect_to_nearest_neighbors(pts, have_l, have_w, radius, k, directed)
    assert np.array_equal(to_np(g.edges.tensor), wl) and np.array_equal(to_np(g.edge_weights), ww)
    assert np.array_equal(to_np(g.edge_index_offsets), wo)
    if not directed:
        keys = set(map(tuple, wl.tolist()))
        assert all((b, a) in keys for a, b in keys)                   # symmetric although the lists were cut
    m = len(wl)
    g.connect_to_nearest_neighbors(radius, k)                         # nothing new the second time
    assert len(g.edges) == m


def test_add_node_and_connect_is_strict(eng):
    from cupoch_amd import geometry
    pts = np.array([[0, 0, 0], [0.5, 0, 0], [2, 0, 0], [1, 1, 0]], F)
    for directed in (True, False):
        g = geometry.Graph(pts)
        g.is_directed = directed
        g.add_edge((0, 2), 3.0)
        l0, w0 = to_np(g.edges.tensor).copy(), to_np(g.edge_weights).copy()
        g.add_node_and_connect((1, 0, 0), 1.0)       # node 0 and node 2 and node 3 at exactly 1.0: not joined; node 1 at 0.5 is
        _, wl, ww = gx.add_node_and_connect(pts, l0, w0, (1, 0, 0), 1.0, directed)
        wl, ww, _, wo = gx.construct(wl, 5, ww)
        assert len(wl) == len(l0) + (1 if directed else 2)
        assert np.array_equal(to_np(g.edges.tensor), wl) and np.array_equal(to_np(g.edge_weights), ww)
        assert np.array_equal(to_np(g.edge_index_offsets), wo) and len(g.points) == 5
        g.add_node_and_connect((1, 0, 0), float(np.nextafter(F(1), F(2))), lazy_add=True)
        assert not g.is_constructed() and len(g.edges) == len(wl) + (5 if directed else 10)   # now all five, the twin at distance 0 too


@pytest.mark.parametrize("res", [(1, 1, 1), (1, 1, 4), (2, 1, 3), (4, 3, 2), (12, 9, 7)])
def test_lattice_equals_the_restatement(eng, res):
    from cupoch_amd import geometry
    lo, hi = (-1.0, -2.0, 0.5), (1.0, 1.0, 2.0)
    pts, lines, w, off = gx.lattice(lo, hi, res)
    g = geometry.Graph.create_from_axis_aligned_bounding_box(lo, hi, res)
    assert to_np(g.points.tensor).tobytes() == pts.tobytes()
    assert np.array_equal(to_np(g.edges.tensor).reshape(-1, 2), lines) and to_np(g.edge_weights).tobytes() == w.tobytes()
    assert np.array_equal(to_np(g.edge_index_offsets), off) and (g.is_constructed() or len(lines) == 0)
    g2 = geometry.Graph.create_from_axis_aligned_bounding_box(geometry.AxisAlignedBoundingBox(lo, hi), res)
    assert to_np(g2.points.tensor).tobytes() == pts.tobytes() and np.array_equal(to_np(g2.edges.tensor).reshape(-1, 2), lines)
    p, l, ww, o = eng.graph_lattice(lo, hi, res)              # the raw entry; then the capacity rule
    assert np.array_equal(to_np(l).reshape(-1, 2), lines) and np.array_equal(to_np(o), off)
    from cupoch_amd import MiIcpError
    with pytest.raises(MiIcpError):
        eng.graph_lattice(lo, hi, (res[0], 0, res[2]))
