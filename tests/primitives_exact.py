"""Case tables and references for the exact tests of the device primitives (csrc/primitives.h: radix sort, exclusive
scan) and of the Morton order on top of them.  tests/test_primitives_cpu.py holds this module against plain Python and
the tile tables against the library's own plan; tests/test_gpu_0_primitives.py holds the kernels against it.  numpy
only; everything is integer work, every comparison is bit for bit, no case skips or samples elements.

The sort's contract as pinned here
  * pairs (radix_sort_pairs<uint64_t> / <uint32_t>, `key_bits`): ceil(key_bits / 8) passes of one byte each, so the
    bytes that are SORTED are the low 8 * ceil(key_bits / 8) bits of the key (`pair_mask`), not the low key_bits bits:
    a caller whose keys have bits between key_bits and the next byte boundary gets them sorted too.
  * the bits ABOVE that mask are ignored: they travel with their element and do not influence the order
    (family `high-garbage`).
  * the sort is STABLE: elements of equal masked key keep their input order, which is what `vals = arange(n)` and the
    heavy duplicates of every family make visible.  The result is exactly keys[order], vals[order] with
    order = argsort(keys & mask, kind="stable").
  * payload (radix_sort_payload32, `lo_bit`, `hi_bit`): passes at shifts lo_bit, lo_bit + 8, ... below hi_bit, each
    on one byte; with keys below 2^hi_bit that is the stable order of keys >> lo_bit.  The low lo_bit bits travel and
    do not influence the order; the key and every present float3 array are permuted alike, 12 bytes per element,
    moved as bits (NaN payloads and -0 included).  lo_bit == hi_bit is no pass: the input comes back unchanged.
  * which tile size runs depends on n alone (the tables below name it per size; mi_icp_debug_sort_plan reports it
    and every GPU case asserts the report first).  The pair rows hold the plan's words [0..2]: on the one-launch
    "whole" path (n <= 65536) the kernel runs tiles of 2048 whatever the tier's chunks and segments say.
Not covered: exclusive_scan_u32 with out != in (the out-of-place scan) is reachable only through mi_knn; the debug
entry point scans in place.  voxel_wide_sort (11-bit digits, voxel_dense.h) has its own plan-asserted voxel cases.

The Morton reference restates csrc/lbvh.h:106-138 (spread3, morton_keys: cell = trunc((p - min) * 2^bits / extent)
clamped to [0, 2^bits - 1], key = x << 2 | y << 1 | z interleaved, x in the highest bit of every triple) and
csrc/mi_build.hip:23-30 (morton_bits_for).  On `morton_lattice` clouds -- coordinates k / 1024, both corners present,
so min = 0, extent = 1 and the scale a power of two -- every fp32 step of morton_keys is exact."""
import ctypes as C

import numpy as np

U32, U64 = np.uint32, np.uint64

# ---- the tile tables, restated (csrc/primitives.h kPairTiers / kPayTiers / kSortWholeMax) ---------------------------
WHOLE_MAX = 1 << 16
PAIR_STARTS = (1 << 18, 1 << 21)
PAY_STARTS = (1 << 18, 1 << 20)


def plan_restated(n):
    """(whole, pair chunks, pair segments, payload chunks, payload segments) -- the tier tables in four lines"""
    pair = 16 if n >= 1 << 21 else 4 if n >= 1 << 18 else 1
    pay = 8 if n >= 1 << 20 else 4 if n >= 1 << 18 else 1
    return (int(n <= WHOLE_MAX), pair, -(-n // (512 * pair)), pay, -(-n // (512 * pay)))


def sort_plan(n):
    """mi_icp_debug_sort_plan(n) as a tuple of 8 ints (no GPU, no context)"""
    from cupoch_amd import _lib
    out = (C.c_int32 * 8)()
    rc = _lib.load().mi_icp_debug_sort_plan(int(n), out)
    assert rc == 0, rc
    return tuple(out)


# ---- sizes: every row names the plan it was written for -------------------------------------------------------------
# (n, whole, chunks, segments)
PAIR_SIZES = [
    (1, 1, 1, 1), (64, 1, 1, 1), (65, 1, 1, 1), (2047, 1, 1, 4), (2048, 1, 1, 4), (2049, 1, 1, 5),
    (65535, 1, 1, 128), (65536, 1, 1, 128),                                        # whole: tiles of 2048
    (65537, 0, 1, 129), (65536 + 512, 0, 1, 129), ((1 << 18) - 1, 0, 1, 512),      # 1 chunk: tiles of 512
    (1 << 18, 0, 4, 128), ((1 << 18) + 2049, 0, 4, 130), ((1 << 21) - 1, 0, 4, 1024),   # 4 chunks: 2048
    (1 << 21, 0, 16, 256), ((1 << 21) + 8193, 0, 16, 258),                         # 16 chunks: 8192
]
# (n, chunks, segments)
PAY_SIZES = [
    (1, 1, 1), (511, 1, 1), (512, 1, 1), (513, 1, 2), ((1 << 18) - 1, 1, 512),     # 1 chunk: tiles of 512
    (1 << 18, 4, 128), ((1 << 18) + 2049, 4, 130), ((1 << 20) - 1, 4, 512),        # 4 chunks: 2048
    (1 << 20, 8, 256), ((1 << 20) + 4097, 8, 258),                                 # 8 chunks: 4096
]
CROSS_MAX = 65537          # all families x all widths up to here; above: every family once, widths alternating
SUBSETS_MAX = 1 << 18      # all payload array subsets up to here; above: points only, all three

FAMILIES = ["random", "constant", "lane-distinct", "two-bins", "sorted", "reversed", "tile-skew"]
PAIR_FAMILIES = FAMILIES + ["high-garbage"]
WIDTHS64 = [1, 8, 9, 33, 64]
WIDTHS32 = [1, 8, 17, 32]
WINDOWS = [(0, 8), (5, 21), (0, 24), (3, 32), (7, 7)]
# one width with an odd and one with an even number of passes: both ping-pong buffers return a result
LARGE_WIDTHS64 = [33, 64]          # 5, 8 passes
LARGE_WIDTHS32 = [17, 32]          # 3, 4 passes
LARGE_WINDOWS = [(0, 24), (3, 32)]  # 3, 4 passes
ALL_SUBSETS = [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]   # () = keys only
LARGE_SUBSETS = [(0,), (0, 1, 2)]


def pair_mask(key_bits):
    """the bits the passes sort: whole bytes"""
    return (1 << (8 * ((key_bits + 7) // 8))) - 1


def pair_tile(row):
    n, whole, chunks, _ = row
    return 2048 if whole else 512 * chunks


def _has_room_above(width, key_width):
    return 8 * ((width + 7) // 8) < key_width


def pair_cases(key_width):
    """[(row, family, key_bits)] for the 64- or 32-bit pair sort.  high-garbage only where bits exist above the mask
    (not at the full key width)."""
    widths, large = (WIDTHS64, LARGE_WIDTHS64) if key_width == 64 else (WIDTHS32, LARGE_WIDTHS32)
    garbage_large = [w for w in large if _has_room_above(w, key_width)]
    out = []
    for row in PAIR_SIZES:
        for f, fam in enumerate(PAIR_FAMILIES):
            if row[0] <= CROSS_MAX:
                ws = widths
            elif fam == "high-garbage":
                ws = garbage_large[:1]
            else:
                ws = [large[(f + row[3]) % 2]]
            for w in ws:
                if fam == "high-garbage" and not _has_room_above(w, key_width):
                    continue
                out.append((row, fam, w))
    return out


def payload_cases():
    """[(row, family, (lo, hi))]; the array subsets are looped inside a case (`payload_subsets`)"""
    out = []
    for row in PAY_SIZES:
        for f, fam in enumerate(FAMILIES):
            wins = WINDOWS if row[0] <= CROSS_MAX else [LARGE_WINDOWS[(f + row[2]) % 2]]
            out += [(row, fam, w) for w in wins]
    return out


def payload_subsets(n):
    return ALL_SUBSETS if n <= SUBSETS_MAX else LARGE_SUBSETS


# ---- key families ---------------------------------------------------------------------------------------------------
def _rep(d):
    """the byte d in every byte of a 64-bit word: whichever byte a pass sorts, its digit is d"""
    return np.asarray(d, U64) * U64(0x0101010101010101)


def field(family, n, tile, seed, bits):
    """n values below 2^bits (uint64) of a family; the sorted part of a key.  Every family has heavy duplicates."""
    rng = np.random.default_rng(seed)
    top = U64((1 << bits) - 1)
    i = np.arange(n, dtype=U64)

    def rand(m):
        r = rng.integers(0, 1 << 64, m, dtype=U64) & top
        r[: m // 2] %= U64(97)                           # plenty of duplicates: stability must show
        return r[rng.permutation(m)] if m else r

    if family in ("random", "high-garbage"):
        return rand(n)
    if family == "constant":                             # one bin holds every tile whole
        return np.full(n, _rep(0xA5) & top, U64)
    if family == "lane-distinct":                        # every lane of a wave its own digit, spread over the bins
        return _rep((i % U64(64)) * U64(4)) & top
    if family == "two-bins":                             # alternating
        return np.where(i % U64(2) == 0, _rep(0x33), _rep(0xCC)) & top
    if family == "sorted":
        return np.sort(rand(n))
    if family == "reversed":
        return np.sort(rand(n))[::-1].copy()
    if family == "tile-skew":                            # the first tile whole in the LAST bin: the largest gdelta
        r = rand(n)
        r[:tile] = _rep(0xFF) & top
        return r
    raise ValueError(family)


def pair_keys(family, n, tile, seed, key_bits, key_width):
    """keys of the pair sort: the family's field in the low key_bits bits; high-garbage sets random bits above the
    sorted bytes"""
    k = field(family, n, tile, seed, key_bits)
    if family == "high-garbage":
        m = pair_mask(key_bits)
        assert m < (1 << key_width) - 1
        g = np.random.default_rng(seed + 1).integers(0, 1 << 64, n, dtype=U64)
        k |= g & U64(((1 << key_width) - 1) & ~m)
    return k.astype(U64 if key_width == 64 else U32)


def payload_keys(family, n, tile, seed, lo, hi):
    """uint32 keys below 2^hi: the family's field in the bits [lo, hi), random bits below lo"""
    k = field(family, n, tile, seed, hi - lo) << U64(lo)
    k |= np.random.default_rng(seed + 2).integers(0, 1 << lo, n, dtype=U64)
    assert n == 0 or int(k.max()) < (1 << hi)
    return k.astype(U32)


def payload_array(n, which):
    """(n, 3) float32 of distinct bit patterns (an odd multiplier permutes the 32-bit words; about one in 256 is a
    NaN pattern of its own), with -0 and two NaN patterns planted: a float compare or a move that is not 12 bytes per
    element shows"""
    w = (np.arange(3 * n, dtype=U64) * U64(2654435761) + U64(0x9E3779B9) * U64(which + 1)) & U64(0xffffffff)
    w = w.astype(U32)
    for pos, pat in ((0, 0x80000000), (3 * n // 2, 0x7fc00001), (3 * n - 1, 0xffc00000)):
        w[pos] = pat
    return w.view(np.float32).reshape(n, 3)


# ---- references and the comparisons the GPU tests use ---------------------------------------------------------------
def ref_pair_order(keys, key_bits):
    return np.argsort(keys & keys.dtype.type(pair_mask(key_bits) & ((1 << (8 * keys.itemsize)) - 1)), kind="stable")


def ref_payload_order(keys, lo):
    return np.argsort(keys.astype(U64) >> U64(lo), kind="stable")


def _first_bad(got, want):
    bad = np.flatnonzero(np.asarray(got).reshape(len(want), -1) != np.asarray(want).reshape(len(want), -1))
    return int(bad[0]) if len(bad) else -1


def check_pairs(got_keys, got_vals, keys, vals, key_bits):
    """raises AssertionError unless (got_keys, got_vals) is the stable sort of (keys, vals), bit for bit"""
    order = ref_pair_order(keys, key_bits)
    assert got_keys.dtype == keys.dtype and got_keys.shape == keys.shape and got_vals.shape == vals.shape
    assert np.array_equal(got_keys, keys[order]), "keys differ, first at %d" % _first_bad(got_keys, keys[order])
    assert np.array_equal(got_vals, vals[order]), "vals differ (stability), first at %d" % _first_bad(got_vals, vals[order])


def check_payload(got_keys, got_arrays, keys, arrays, lo):
    """the same for the payload sort: arrays are (n, 3) float32 or None, compared as uint32 views"""
    order = ref_payload_order(keys, lo)
    assert got_keys.dtype == U32 and got_keys.shape == keys.shape
    assert np.array_equal(got_keys, keys[order]), "keys differ, first at %d" % _first_bad(got_keys, keys[order])
    for a, (g, w) in enumerate(zip(got_arrays, arrays)):
        assert (g is None) == (w is None)
        if w is None:
            continue
        want = w[order].view(U32)
        assert g.shape == w.shape
        assert np.array_equal(g.view(U32), want), "array %d differs, first at row %d" % (a, _first_bad(g.view(U32), want))


# ---- calls ----------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def gpu_sort_pairs(eng, keys, vals, key_bits, check=True):
    """the 64- or 32-bit entry point by the keys' dtype; returns (rc, keys, vals)"""
    k, v = keys.copy(), np.ascontiguousarray(vals, U32).copy()
    fn = eng._L.mi_icp_debug_sort_pairs if k.dtype == U64 else eng._L.mi_icp_debug_sort_pairs32
    rc = fn(eng._ctx, _ptr(k), _ptr(v), len(k), key_bits)
    if check:
        eng._chk(rc)
    return rc, k, v


def gpu_sort_payload(eng, keys, arrays, lo, hi, check=True):
    k = keys.copy()
    arr = [None if a is None else a.copy() for a in arrays]
    rc = eng._L.mi_icp_debug_sort_payload32(eng._ctx, _ptr(k), _ptr(arr[0]), _ptr(arr[1]), _ptr(arr[2]), len(k), lo, hi)
    if check:
        eng._chk(rc)
    return rc, k, arr


# ---- scan -----------------------------------------------------------------------------------------------------------
SCAN_TILE = 2048       # kScanTile
# (n, reaches): values below 2^16 can bring the total of n elements into [2^31, 2^32) only for n > ~36000; the sizes
# below that run the family's full 16-bit range and the reference side asserts their total stays below 2^31
SCAN_SIZES = [(1, False), (7, False), (255, False), (256, False), (2047, False), (2048, False), (2049, False),
              (5000, False), (8191, False), (8192, False), (8193, False), (40000, True), (65535, True), (65536, True),
              (65537, True), (70000, True), (4194304 + 17, True)]


def scan_values(n, reaches, seed):
    """uint32 values below 2^16 whose total lies in [2^31, 2^32) where n can reach it: uniform in [lo, hi) with the
    mean at 1.1 * 2^31 / n and hi <= 1.9 * 2^31 / n"""
    rng = np.random.default_rng(seed)
    need = -(-(11 * (1 << 31)) // (10 * n))
    hi = min(1 << 16, (19 * (1 << 31)) // (10 * n))
    lo = max(0, 2 * need - hi)
    if not reaches:
        assert need >= 1 << 16
        lo, hi = 0, 1 << 16
    a = rng.integers(lo, hi, n, dtype=np.int64).astype(U32)
    total = int(a.astype(U64).sum())
    assert ((1 << 31) <= total < (1 << 32)) == reaches, (n, total)
    return a


def scan_sparse(n):
    """all zero but the last element of a tile and the first of the next (the last tile boundary inside n): the two
    add up to 2^32 - 1 with the high bit in the first; None below 2049 elements"""
    t = (n - 1) // SCAN_TILE
    if t < 1:
        return None
    a = np.zeros(n, U32)
    a[t * SCAN_TILE - 1] = 0xC0000000
    a[t * SCAN_TILE] = 0x3FFFFFFF
    return a


def ref_scan(a):
    """(exclusive prefix as uint32, total) from np.cumsum in uint64"""
    c = np.cumsum(a.astype(U64), dtype=U64)
    return np.concatenate([np.zeros(1, U64), c[:-1]]).astype(U32), int(c[-1])


# ---- Morton ---------------------------------------------------------------------------------------------------------
def morton_bits_for(n):
    """csrc/mi_build.hip:23-30"""
    lg = 0
    while (1 << lg) < n:
        lg += 1
    per_axis = (lg + 2) // 3
    fine = min(21, max(6, per_axis + 2))
    coarse = (((3 * fine + 7) // 8 - 1) * 8) // 3
    return coarse if coarse >= max(6, per_axis) else fine


def spread3(v):
    """csrc/lbvh.h:106-114: 21 bits -> every third bit"""
    x = v.astype(U64) & U64(0x1fffff)
    x = (x | x << U64(32)) & U64(0x1f00000000ffff)
    x = (x | x << U64(16)) & U64(0x1f0000ff0000ff)
    x = (x | x << U64(8)) & U64(0x100f00f00f00f00f)
    x = (x | x << U64(4)) & U64(0x10c30c30c30c30c3)
    x = (x | x << U64(2)) & U64(0x1249249249249249)
    return x


def morton_lattice(n, seed):
    """(k, points): n >= 2 lattice points k / 1024, k integer in [0, 1024]^3, both corners present, many repeated"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1025, (n, 3), dtype=np.int64)
    k[n // 3:n // 2] = k[: n // 2 - n // 3]               # exact duplicates: ties keep the input order
    k[rng.integers(0, n)] = 0
    k[-1] = 1024
    if not (k == 0).all(1).any():
        k[0] = 0
    return k, (k.astype(np.float64) / 1024.0).astype(np.float32)


def morton_keys(k, bits):
    """csrc/lbvh.h:119-138 on a lattice cloud: cell = min(floor(k * 2^bits / 1024), 2^bits - 1), x in the highest bit
    of every triple; uint32 keys where 3 * bits <= 32"""
    q = np.minimum((k.astype(np.int64) << bits) >> 10, (1 << bits) - 1)
    key = (spread3(q[:, 0]) << U64(2)) | (spread3(q[:, 1]) << U64(1)) | spread3(q[:, 2])
    return key.astype(U32) if 3 * bits <= 32 else key


# (n, bits given from outside or None for the engine's own choice, the bits that run, key width,
#  the pair sort's plan (whole, chunks, segments))
MORTON_CASES = [
    # the engine's choice (at most 10 bits below 2^30 points: narrow keys): whole, whole, 1 chunk
    (1000, None, 6, 32, (1, 1, 2)), (20000, None, 7, 32, (1, 1, 40)), (200000, None, 8, 32, (0, 1, 391)),
    # bits given: the widest narrow key, the wide keys in the 1-chunk and the 4-chunk tier
    (70000, 10, 10, 32, (0, 1, 137)), (70000, 11, 11, 64, (0, 1, 137)), (300000, 21, 21, 64, (0, 4, 147)),
]
