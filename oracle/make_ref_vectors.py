#!/usr/bin/env python3
"""Record what the reference's own libraries (oracle/_ref, built by `make _ref`) answer on the inputs of two tests,
so that those tests run where oracle/_ref cannot be built:

* tests/golden/ref_lzf_streams.npz -- for every case of lzf_cases(): `ref_<i>`, the stream the reference's vendored
  liblzf writes, and `eng_<i>`, the stream cupoch_amd.io.lzf_compress writes, recorded only once the reference's
  lzf_decompress has turned it back into the input (tests/test_io_and_real_data.py).
* tests/golden/ref_flann_search.npz -- the reference's FLANN CPU kd-tree on flann_inputs(): the golden k-NN case of
  reference_tests.json and the 5-NN / radius searches (tests/test_oracle_selfcheck.py).

Run from anywhere once build() has made oracle/_ref; only the recorded DATA is committed.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LZF_VECTORS = os.path.join(GOLDEN, "ref_lzf_streams.npz")
FLANN_VECTORS = os.path.join(GOLDEN, "ref_flann_search.npz")
FLANN_RADIUS, FLANN_MAX_NN = 0.02, 3


def lzf_cases():
    """The byte strings the LZF test exchanges with the reference's liblzf."""
    rng = np.random.default_rng(3)
    pts = rng.random((4000, 3), dtype=np.float32)
    return [b"a" * 5, bytes(rng.integers(0, 256, 20000, dtype=np.uint8)), np.repeat(rng.random(700, dtype=np.float32), 5).tobytes(),
            bytes(70000), b"0123456789" * 2500, np.ascontiguousarray(pts.T).tobytes(),          # field-major floats: a PCD payload
            np.round(pts * 64).astype(np.float32).T.tobytes()]


def flann_inputs():
    """(target, queries) of the FLANN comparison."""
    rng = np.random.default_rng(1)
    tgt = rng.random((20000, 3), dtype=np.float32)
    qry = rng.random((2000, 3), dtype=np.float32)
    return tgt, qry


def main():
    sys.path.insert(0, ROOT)
    from cupoch_amd.io import lzf_compress
    from oracle import oracle as orc
    L = orc.ref_lzf()
    if L is None or not orc.ref_flann_available():
        sys.exit("oracle/_ref is not built: run build() where the reference checkout exists")
    out = {}
    for i, data in enumerate(lzf_cases()):
        cap = len(data) * 2 + 64
        buf = C.create_string_buffer(cap)
        n = L.lzf_compress(data, len(data), buf, cap)
        assert n > 0
        comp = lzf_compress(data)
        dec = C.create_string_buffer(len(data) + 16)
        m = L.lzf_decompress(comp, len(comp), dec, len(data) + 16)
        assert m == len(data) and dec.raw[:m] == data, "the reference does not decode case %d" % i
        out["ref_%d" % i] = np.frombuffer(buf.raw[:n], np.uint8)
        out["eng_%d" % i] = np.frombuffer(comp, np.uint8)
    np.savez_compressed(LZF_VECTORS, **out)

    g = json.load(open(os.path.join(GOLDEN, "reference_tests.json")))["kdtree_search_knn"]
    gi, _ = orc.ref_flann_knn(g["points"], [g["query"]], g["knn"])
    tgt, qry = flann_inputs()
    ki, kd = orc.ref_flann_knn(tgt, qry, 5)
    r, ri, rd = orc.ref_flann_radius(tgt, qry, FLANN_RADIUS, FLANN_MAX_NN)
    np.savez_compressed(FLANN_VECTORS, golden_knn_idx=gi[0], knn_idx=ki, knn_d2=kd,
                        radius_count=np.array([r], np.int64), radius_idx=ri, radius_d2=rd)
    print("wrote", LZF_VECTORS, FLANN_VECTORS)


if __name__ == "__main__":
    main()
