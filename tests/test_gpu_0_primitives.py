"""GPU: the hand-written device primitives behind the engine (radix sort, scan,
Morton order) against numpy -- bit-exact integer work.  The second half runs the tables of tests/primitives_exact.py:
every tile size of every sort form, each case asserting first that its size still takes the path its row names."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _sort(eng, keys, vals, bits):
    k = np.ascontiguousarray(keys, np.uint64).copy()
    v = np.ascontiguousarray(vals, np.uint32).copy()
    eng._chk(eng._L.mi_icp_debug_sort_pairs(eng._ctx, k.ctypes.data_as(C.c_void_p),
                                            v.ctypes.data_as(C.c_void_p), len(k), bits))
    return k, v


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 100003, 3000000])
@pytest.mark.parametrize("bits", [8, 24, 39, 64])
def test_radix_sort_is_a_stable_sort(eng, n, bits):
    rng = np.random.default_rng(n * 131 + bits)
    hi = (1 << bits) - 1
    keys = rng.integers(0, 1 << 62, n, dtype=np.uint64) & np.uint64(hi)
    if n > 1000:                       # plenty of duplicates: stability must show
        keys[: n // 2] = keys[: n // 2] % np.uint64(97)
    vals = np.arange(n, dtype=np.uint32)
    k, v = _sort(eng, keys, vals, bits)
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(k, keys[order])
    np.testing.assert_array_equal(v, vals[order])


@pytest.mark.parametrize("n", [1, 7, 255, 256, 2047, 2048, 2049, 5000, 8191, 8192, 8193, 40000, 65535, 65536, 65537, 70000, 4194304 + 17])
def test_exclusive_scan(eng, n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 5, n, dtype=np.uint32)
    out = np.empty_like(a)
    tot = C.c_uint64(0)
    eng._chk(eng._L.mi_icp_debug_exclusive_scan(eng._ctx, a.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p), n, C.byref(tot)))
    ref = np.concatenate([[0], np.cumsum(a.astype(np.uint64))[:-1]]).astype(np.uint32)
    np.testing.assert_array_equal(out, ref)
    assert tot.value == int(a.astype(np.uint64).sum())


def test_morton_order_is_a_permutation_and_coherent(eng):
    rng = np.random.default_rng(3)
    n = 200000
    pts = rng.random((n, 3), dtype=np.float32)
    order = np.empty(n, np.uint32)
    eng._chk(eng._L.mi_icp_debug_morton_order(eng._ctx, pts.ctypes.data_as(C.c_void_p), n,
                                              order.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
    sp = pts[order]
    # 64 consecutive points of the order form a compact blob: extent far below the cloud's
    ext = (sp[: n // 64 * 64].reshape(-1, 64, 3).max(1) - sp[: n // 64 * 64].reshape(-1, 64, 3).min(1)).max(1)
    assert np.median(ext) < 0.15


# ---- every tier, key width and payload form, bit for bit (tables and references: tests/primitives_exact.py) ----------
import primitives_exact as px  # noqa: E402


def _pair_id(case):
    return "%d-%s-%d" % (case[0][0], case[1], case[2])


def _run_pairs(eng, case, key_width):
    row, family, bits = case
    n = row[0]
    plan = px.sort_plan(n)
    tile = px.pair_tile(row)
    print("pairs%d n=%d family=%s key_bits=%d passes=%d plan: whole=%d chunks=%d segments=%d hist=%d -> tile %d%s"
          % (key_width, n, family, bits, (bits + 7) // 8, plan[0], plan[1], plan[2], plan[5], tile,
             " (one launch per pass)" if plan[0] else ""))
    assert plan[:3] == row[1:], "this size no longer runs the path its row names"
    keys = px.pair_keys(family, n, tile, 7 * n + bits, bits, key_width)
    vals = np.arange(n, dtype=np.uint32)
    _, k, v = px.gpu_sort_pairs(eng, keys, vals, bits)
    px.check_pairs(k, v, keys, vals, bits)


@pytest.mark.parametrize("case", px.pair_cases(64), ids=_pair_id)
def test_pairs64_exact(eng, case):
    _run_pairs(eng, case, 64)


@pytest.mark.parametrize("case", px.pair_cases(32), ids=_pair_id)
def test_pairs32_exact(eng, case):
    _run_pairs(eng, case, 32)


@pytest.mark.parametrize("case", px.payload_cases(), ids=lambda c: "%d-%s-%d.%d" % (c[0][0], c[1], c[2][0], c[2][1]))
def test_payload_exact(eng, case):
    row, family, (lo, hi) = case
    n = row[0]
    plan = px.sort_plan(n)
    print("payload n=%d family=%s bits=[%d, %d) passes=%d plan: chunks=%d segments=%d hist=%d -> tile %d"
          % (n, family, lo, hi, (hi - lo + 7) // 8, plan[3], plan[4], plan[5], 512 * plan[3]))
    assert plan[3:5] == row[1:], "this size no longer runs the path its row names"
    keys = px.payload_keys(family, n, 512 * row[1], 11 * n + lo + hi, lo, hi)
    full = [px.payload_array(n, a) for a in range(3)]
    for subset in px.payload_subsets(n):
        arrays = [full[a] if a in subset else None for a in range(3)]
        _, k, got = px.gpu_sort_payload(eng, keys, arrays, lo, hi)
        px.check_payload(k, got, keys, arrays, lo)


def test_descending_sizes_on_one_context():
    """The buffers are sized by the first, largest sort; the second needs the most histogram segments (1024 tiles of
    2048 against the first's 258 of 8192)."""
    from cupoch_amd.engine import Engine
    e = Engine(0)
    try:
        sizes = [(1 << 21) + 8193, (1 << 21) - 1, 65537, 2049]
        plans = [px.sort_plan(n) for n in sizes]
        print("descending: " + ", ".join("n=%d segments=%d of hist=%d" % (n, p[2], plans[0][5]) for n, p in zip(sizes, plans)))
        assert plans[1][2] == plans[0][5] == 1024 > plans[0][2]
        for n in sizes:
            for key_width, bits in ((64, 33), (32, 32)):
                keys = px.pair_keys("random", n, 512, n + key_width, bits, key_width)
                vals = np.arange(n, dtype=np.uint32)
                _, k, v = px.gpu_sort_pairs(e, keys, vals, bits)
                px.check_pairs(k, v, keys, vals, bits)
            keys = px.payload_keys("random", n, 512, n, 0, 24)
            arrays = [px.payload_array(n, 0), None, None]
            _, k, got = px.gpu_sort_payload(e, keys, arrays, 0, 24)
            px.check_payload(k, got, keys, arrays, 0)
    finally:
        e.close()


def test_argument_errors_leave_the_context_usable(eng):
    from cupoch_amd import _lib
    n = 3000
    keys = px.pair_keys("random", n, 512, 5, 17, 32)
    vals = np.arange(n, dtype=np.uint32)
    L, ctx, P = eng._L, eng._ctx, px._ptr
    for bits in (0, -1, 33):
        assert px.gpu_sort_pairs(eng, keys, vals, bits, check=False)[0] == _lib.MI_ICP_ERR_INVALID
    k, v = keys.copy(), vals.copy()
    assert L.mi_icp_debug_sort_pairs32(ctx, P(k), P(v), -1, 17) == _lib.MI_ICP_ERR_INVALID
    assert L.mi_icp_debug_sort_pairs32(ctx, None, P(v), n, 17) == _lib.MI_ICP_ERR_INVALID
    assert L.mi_icp_debug_sort_pairs32(ctx, P(k), None, n, 17) == _lib.MI_ICP_ERR_INVALID
    assert np.array_equal(k, keys) and np.array_equal(v, vals)
    _, k, v = px.gpu_sort_pairs(eng, keys, vals, 17)
    px.check_pairs(k, v, keys, vals, 17)

    pkeys = px.payload_keys("random", n, 512, 6, 5, 21)
    arrays = [px.payload_array(n, 0), None, px.payload_array(n, 2)]
    for lo, hi in ((-1, 8), (0, 33), (9, 8), (33, 33), (-2, -1)):
        rc, k, got = px.gpu_sort_payload(eng, pkeys, arrays, lo, hi, check=False)
        assert rc == _lib.MI_ICP_ERR_INVALID, (lo, hi)
        assert np.array_equal(k, pkeys) and np.array_equal(got[0].view(np.uint32), arrays[0].view(np.uint32))
    k = pkeys.copy()
    assert L.mi_icp_debug_sort_payload32(ctx, None, None, None, None, n, 5, 21) == _lib.MI_ICP_ERR_INVALID
    assert L.mi_icp_debug_sort_payload32(ctx, P(k), None, None, None, -1, 5, 21) == _lib.MI_ICP_ERR_INVALID
    _, k, got = px.gpu_sort_payload(eng, pkeys, arrays, 5, 21)
    px.check_payload(k, got, pkeys, arrays, 5)
    # lo == hi at both ends is a legal no-pass call
    for b in (0, 32):
        _, k, got = px.gpu_sort_payload(eng, pkeys, arrays, b, b)
        assert np.array_equal(k, pkeys)
        for g, a in zip(got, arrays):
            assert (g is None and a is None) or np.array_equal(g.view(np.uint32), a.view(np.uint32))


def _scan(eng, a):
    out = np.empty_like(a)
    tot = C.c_uint64(0)
    eng._chk(eng._L.mi_icp_debug_exclusive_scan(eng._ctx, a.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p), len(a), C.byref(tot)))
    return out, tot.value


@pytest.mark.parametrize("n,reaches", px.SCAN_SIZES)
def test_exclusive_scan_large_values(eng, n, reaches):
    a = px.scan_values(n, reaches, n)                       # (asserts where the total lies)
    ref, total = px.ref_scan(a)
    print("scan n=%d tiles=%d total=%d (2^31 <= total < 2^32: %s)" % (n, -(-n // px.SCAN_TILE), total, reaches))
    out, tot = _scan(eng, a)
    np.testing.assert_array_equal(out, ref)
    assert tot == total
    s = px.scan_sparse(n)
    if s is not None:                                       # one value at the end of a tile, one at the start of the next
        ref, total = px.ref_scan(s)
        out, tot = _scan(eng, s)
        np.testing.assert_array_equal(out, ref)
        assert tot == total == (1 << 32) - 1


@pytest.mark.parametrize("n,given,bits,width,declared", px.MORTON_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_morton_order_on_a_lattice_is_the_stable_sort_of_the_keys(eng, n, given, bits, width, declared):
    plan = px.sort_plan(n)
    assert plan[:3] == declared, "this size no longer runs the path its row names"
    k, pts = px.morton_lattice(n, n)
    order = np.empty(n, np.uint32)
    if given is None:
        assert px.morton_bits_for(n) == bits
        eng._chk(eng._L.mi_icp_debug_morton_order(eng._ctx, pts.ctypes.data_as(C.c_void_p), n,
                                                  order.ctypes.data_as(C.c_void_p)))
    else:
        eng._chk(eng._L.mi_icp_debug_morton_order_bits(eng._ctx, pts.ctypes.data_as(C.c_void_p), n, given,
                                                       order.ctypes.data_as(C.c_void_p)))
    keys = px.morton_keys(k, bits)
    print("morton n=%d bits=%d (%s) key width=%d passes=%d plan: whole=%d chunks=%d segments=%d"
          % (n, bits, "given" if given else "the engine's choice", 8 * keys.itemsize, (3 * bits + 7) // 8, plan[0], plan[1], plan[2]))
    assert 8 * keys.itemsize == width
    assert len(np.unique(keys)) < n                          # ties: the input order must be kept
    np.testing.assert_array_equal(order, np.argsort(keys, kind="stable").astype(np.uint32))
