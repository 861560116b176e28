"""No GPU: the sort's tile plan as the library reports it (mi_icp_debug_sort_plan calls the drivers' own functions)
against the tier tables restated, the histogram buffer's size against every sort it must serve, and the references
and comparisons of tests/primitives_exact.py against plain Python -- including that the comparisons CAN fail."""
import numpy as np
import pytest

import primitives_exact as px

TIER_STARTS = sorted(set(px.PAIR_STARTS + px.PAY_STARTS))       # 2^18, 2^20, 2^21


def _plan_sizes():
    s = {1, 2}
    for b in (px.WHOLE_MAX,) + tuple(TIER_STARTS):
        s |= {b - 1, b, b + 1}
        for tile in (512, 2048, 4096, 8192):                    # the tile multiples around the boundary
            for m in (b - tile, b + tile):
                s |= {m - 1, m, m + 1}
    rng = np.random.default_rng(20)
    s |= {int(2 ** e) for e in rng.uniform(0, 27, 200)}         # ~200 seeded sizes up to 2^27, spread over the scales
    s |= {1 << 27}
    return sorted(x for x in s if x >= 1)


PLAN_SIZES = _plan_sizes()


def test_plan_sizes_cover_what_they_claim():
    assert len(PLAN_SIZES) > 250 and PLAN_SIZES[0] == 1 and PLAN_SIZES[-1] == 1 << 27
    for b in [px.WHOLE_MAX] + TIER_STARTS:
        assert {b - 1, b, b + 1} <= set(PLAN_SIZES)


def test_sort_plan_is_the_tier_tables():
    for n in PLAN_SIZES:
        p = px.sort_plan(n)
        assert p[:5] == px.plan_restated(n), n
        assert p[6] == -(-256 * p[5] // px.SCAN_TILE) and p[7] == 0, n


def test_size_tables_name_the_plan_the_library_reports():
    for row in px.PAIR_SIZES:
        assert px.sort_plan(row[0])[:3] == row[1:], row
    for row in px.PAY_SIZES:
        assert px.sort_plan(row[0])[3:5] == row[1:], row
    # every (form, tile) combination has a row
    assert {px.pair_tile(r) for r in px.PAIR_SIZES if r[1]} == {2048}
    assert {px.pair_tile(r) for r in px.PAIR_SIZES if not r[1]} == {512, 2048, 8192}
    assert {512 * r[1] for r in px.PAY_SIZES} == {512, 2048, 4096}


def test_hist_segments_hold_every_smaller_sort():
    """sort_hist_segments(n) sizes the histogram for every sort of m <= n elements, pairs or payload: kd_cell_layout
    sorts S <= n samples in buffers sized for n, and a smaller m may take a smaller tile, hence MORE segments."""
    rng = np.random.default_rng(21)
    for n in PLAN_SIZES:
        hist = px.sort_plan(n)[5]
        peaks = [n] + [b - 1 for b in TIER_STARTS if b - 1 <= n]
        ms = peaks + [int(m) for m in rng.integers(1, n + 1, 100)]
        need = 0
        for m in ms:
            p = px.plan_restated(m)
            assert hist >= p[2] and hist >= p[4], (n, m, hist, p)
            need = max(need, p[2], p[4])
        # ... and no more than that: within a tier the count grows with m, so the most is at n or just below a tier
        assert hist == max(max(px.plan_restated(m)[2], px.plan_restated(m)[4]) for m in peaks), n
        assert hist >= need
    assert px.sort_plan(1 << 21)[5] == 1024 > px.sort_plan(1 << 21)[2]      # the middle size needs the most


def test_sort_plan_rejects_bad_arguments():
    import ctypes as C
    from cupoch_amd import _lib
    L = _lib.load()
    out = (C.c_int32 * 8)()
    assert L.mi_icp_debug_sort_plan(0, out) == _lib.MI_ICP_ERR_INVALID
    assert L.mi_icp_debug_sort_plan(-5, out) == _lib.MI_ICP_ERR_INVALID
    assert L.mi_icp_debug_sort_plan(100, None) == _lib.MI_ICP_ERR_INVALID


def test_case_tables_are_complete():
    for kw, widths in ((64, px.WIDTHS64), (32, px.WIDTHS32)):
        cases = px.pair_cases(kw)
        assert {c[0] for c in cases} == set(px.PAIR_SIZES)
        for row in px.PAIR_SIZES:
            mine = [c for c in cases if c[0] == row]
            assert {c[1] for c in mine} == set(px.PAIR_FAMILIES), row        # no family trimmed at any size
            if row[0] <= px.CROSS_MAX:
                assert {c[2] for c in mine if c[1] != "high-garbage"} == set(widths)
            else:                                                             # both ping-pong parities return a result
                assert {((c[2] + 7) // 8) % 2 for c in mine} == {0, 1}, row
    cases = px.payload_cases()
    for row in px.PAY_SIZES:
        mine = [c for c in cases if c[0] == row]
        assert {c[1] for c in mine} == set(px.FAMILIES)
        if row[0] <= px.CROSS_MAX:
            assert {c[2] for c in mine} == set(px.WINDOWS)
        else:
            assert {((c[2][1] - c[2][0] + 7) // 8) % 2 for c in mine} == {0, 1}, row
    assert len(px.ALL_SUBSETS) == 8 and len(set(px.ALL_SUBSETS)) == 8


# ---- the helper's references against plain Python, and its comparisons against corrupted results ----------------------
SMALL = [1, 2, 3, 17, 64, 65, 130, 257]
TILE = 16


def _swap_equal(keys_sorted, rank):
    """positions (i, i + 1) of two neighbours of equal rank in a sorted result, or None"""
    eq = np.flatnonzero(rank[1:] == rank[:-1])
    return (int(eq[0]), int(eq[0]) + 1) if len(eq) else None


@pytest.mark.parametrize("family", px.PAIR_FAMILIES)
@pytest.mark.parametrize("key_width", [64, 32])
def test_pair_reference_and_its_check(family, key_width):
    widths = px.WIDTHS64 if key_width == 64 else px.WIDTHS32
    swapped = cleared = 0
    for n in SMALL:
        for bits in widths:
            if family == "high-garbage" and px.pair_mask(bits) >= (1 << key_width) - 1:
                continue
            keys = px.pair_keys(family, n, TILE, 1000 * n + bits, bits, key_width)
            assert keys.dtype == (np.uint64 if key_width == 64 else np.uint32) and len(keys) == n
            if family != "high-garbage":
                assert n == 0 or int(keys.max()) < (1 << bits)
            elif n >= 64:
                assert int(keys.max()) > px.pair_mask(bits)                   # the garbage is there
            vals = np.arange(n, dtype=np.uint32)
            mask = px.pair_mask(bits)
            order = sorted(range(n), key=lambda i: int(keys[i]) & mask)       # (Python's sort is stable)
            assert px.ref_pair_order(keys, bits).tolist() == order
            k, v = keys[order], vals[order]
            px.check_pairs(k, v, keys, vals, bits)
            if n > 64:
                assert len(np.unique(keys & keys.dtype.type(mask))) < n       # duplicates: stability is visible
            # two equal-key elements swapped
            sw = _swap_equal(k, k & k.dtype.type(mask))
            if sw:
                k2, v2 = k.copy(), v.copy()
                k2[[sw[0], sw[1]]] = k2[[sw[1], sw[0]]]
                v2[[sw[0], sw[1]]] = v2[[sw[1], sw[0]]]
                with pytest.raises(AssertionError):
                    px.check_pairs(k2, v2, keys, vals, bits)
                swapped += 1
            # a key with its highest set bit cleared (high-garbage: a bit above the sorted bytes)
            j = int(np.argmax(k))
            if int(k[j]) > 0:
                k2 = k.copy()
                k2[j] &= k.dtype.type((1 << (int(k[j]).bit_length() - 1)) - 1)
                with pytest.raises(AssertionError):
                    px.check_pairs(k2, v, keys, vals, bits)
                cleared += 1
    assert swapped >= 10 and cleared >= 10


@pytest.mark.parametrize("family", px.FAMILIES)
def test_payload_reference_and_its_check(family):
    swapped = rows = cleared = 0
    for n in SMALL:
        for lo, hi in px.WINDOWS:
            keys = px.payload_keys(family, n, TILE, 77 * n + lo + hi, lo, hi)
            arrays = [px.payload_array(n, a) for a in range(3)]
            assert len({w for a in arrays for w in a.view(np.uint32).ravel().tolist()}) >= 9 * n - 9   # distinct patterns
            assert np.isnan(arrays[0]).any() and (arrays[1].view(np.uint32) == 0x80000000).any()
            order = sorted(range(n), key=lambda i: int(keys[i]) >> lo)
            assert px.ref_payload_order(keys, lo).tolist() == order
            if lo == hi:
                assert order == list(range(n))                                # no pass: unchanged
            k = keys[order]
            got = [a[order] for a in arrays]
            px.check_payload(k, got, keys, arrays, lo)
            px.check_payload(k, [got[0], None, got[2]], keys, [arrays[0], None, arrays[2]], lo)
            # two equal-key elements swapped (keys with different low bits, and their rows)
            sw = _swap_equal(k, k >> np.uint32(lo))
            if sw:
                k2, g2 = k.copy(), [g.copy() for g in got]
                k2[[sw[0], sw[1]]] = k2[[sw[1], sw[0]]]
                for g in g2:
                    g[[sw[0], sw[1]]] = g[[sw[1], sw[0]]]
                with pytest.raises(AssertionError):
                    px.check_payload(k2, g2, keys, arrays, lo)
                swapped += 1
            # one payload row taken from its neighbour
            if n >= 2:
                for a in range(3):
                    g2 = [g.copy() for g in got]
                    g2[a][n // 2] = g2[a][n // 2 - 1]
                    with pytest.raises(AssertionError):
                        px.check_payload(k, g2, keys, arrays, lo)
                    rows += 1
            # a key with its highest set bit cleared
            if n and int(k.max()) > 0:
                k2 = k.copy()
                j = int(np.argmax(k))
                k2[j] &= np.uint32((1 << (int(k[j]).bit_length() - 1)) - 1)
                with pytest.raises(AssertionError):
                    px.check_payload(k2, got, keys, arrays, lo)
                cleared += 1
    assert swapped >= 10 and rows >= 50 and cleared >= 10


def test_scan_reference_and_value_family():
    for n, reaches in px.SCAN_SIZES:
        if n > 70000:
            continue                                   # (the GPU test builds the large one; the asserts run there)
        a = px.scan_values(n, reaches, n)
        assert a.dtype == np.uint32 and int(a.max()) < 1 << 16
        ref, total = px.ref_scan(a)
        run = 0
        for i in range(0, n, max(1, n // 50)):
            assert int(ref[i]) == sum(int(x) for x in a[:i]) % (1 << 32)
        assert total == sum(int(x) for x in a)
        s = px.scan_sparse(n)
        assert (s is None) == (n <= px.SCAN_TILE)
        if s is not None:
            nz = np.flatnonzero(s)
            assert len(nz) == 2 and nz[1] == nz[0] + 1 and nz[1] % px.SCAN_TILE == 0
            r, t = px.ref_scan(s)
            assert t == (1 << 32) - 1 and int(r[-1]) in (0xC0000000, 0xFFFFFFFF)


def test_morton_reference():
    # morton_bits_for as the table names it, and never wide below 2^30 points
    for n, given, bits, width, plan in px.MORTON_CASES:
        assert (given if given is not None else px.morton_bits_for(n)) == bits
        assert width == (32 if 3 * bits <= 32 else 64)
        assert px.sort_plan(n)[:3] == plan
    assert {c[3] for c in px.MORTON_CASES} == {32, 64}
    assert max(px.morton_bits_for(n) for n in (1, 1000, 10 ** 7, 1 << 27, 1 << 30)) == 10
    assert px.morton_bits_for(10 ** 7) == 8                                    # (24-bit keys, 3 passes: mi_build.hip)
    # the interleave against a bit-by-bit loop
    k, pts = px.morton_lattice(500, 4)
    assert pts.dtype == np.float32 and pts.min() == 0.0 and pts.max() == 1.0
    assert (pts.astype(np.float64) * 1024 == k).all()
    assert (k == 0).all(1).any() and (k == 1024).all(1).any()
    for bits in (6, 10, 11, 21):
        keys = px.morton_keys(k, bits)
        assert keys.dtype == (np.uint32 if 3 * bits <= 32 else np.uint64)
        for i in range(0, 500, 7):
            q = [min(int(c) * (1 << bits) // 1024, (1 << bits) - 1) for c in k[i]]
            want = 0
            for b in range(bits):
                want |= ((q[0] >> b) & 1) << (3 * b + 2) | ((q[1] >> b) & 1) << (3 * b + 1) | ((q[2] >> b) & 1) << (3 * b)
            assert int(keys[i]) == want
