"""Times of feature matching and FastGlobalRegistration, device events around 20 calls after 3 warm-up
calls, the median of 5 such windows:
  mi_icp_feature_match at 20k x 20k x 33 and at 5k x 5k x 352, with the match kernel's share of the fp32 vector peak --
  two lane-operations (a subtraction and a fused multiply-add) per pair and dimension over 78.6e12 lane-operations a
  second (157.3 TFLOPS counts a fused multiply-add as two);
  the whole call on 20k-point clouds with the default option (33 dimensions), host wall time around a synchronised call.
The reference's own formulation (a materialised ref x query matrix, twice) cannot be timed beside it: it is not part of
this library, and at 100k x 100k it does not fit in memory.  Prints one line per row.

    python scripts/dev/fgr_rows.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PEAK_LANE_OPS = 157.3e12 / 2.0


def scene(n, dim, seed=0):
    """two overlapping, permuted copies of a cloud (the second one moved) with noisy copies of its descriptors"""
    rng = np.random.default_rng(seed)
    base = rng.uniform([3.0, 1.0, 2.0], [7.0, 3.0, 3.0], (n + n // 4, 3))
    desc = rng.standard_normal((len(base), dim))
    si, ti = rng.permutation(n), (n // 4 + rng.permutation(n))
    a, ax = 1.1, np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, (0.7, -1.3, 0.4)
    f = lambda x: np.ascontiguousarray(x, np.float32)
    return (f(base[si]), f(base[ti] @ R.T + T[:3, 3]), f(desc[si] + 0.05 * rng.standard_normal((n, dim))),
            f(desc[ti] + 0.05 * rng.standard_normal((n, dim))), T)


def event_ms(fn, calls=20, windows=5):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    import ctypes as C
    import torch
    from cupoch_amd.engine import Engine
    eng = Engine(0)
    L, ctx = eng._L, eng._ctx
    p = lambda t: C.c_void_p(t.data_ptr())
    for n, dim in ((20000, 33), (5000, 352)):
        rng = np.random.default_rng(dim)
        q = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).cuda()
        r = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).cuda()
        qi, ri = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        qd, rd = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
        call = lambda: L.mi_icp_feature_match(ctx, p(q), n, p(r), n, dim, p(qi), p(qd), p(ri), p(rd))
        assert call() == 0
        ms, lo, hi = event_ms(call)
        ops = 2.0 * n * n * dim
        print("feature_match %6d x %6d x %3d   %8.3f ms (windows %.3f .. %.3f)   %.1f%% of the fp32 vector peak, memset and decode "
              "included" % (n, n, dim, ms, lo, hi, 100.0 * ops / (ms * 1e-3) / PEAK_LANE_OPS), flush=True)
    src, tgt, fs, ft, T = scene(20000, 33)
    dev = [torch.from_numpy(a).cuda() for a in (src, tgt, fs, ft)]
    run = lambda: eng.fast_global_registration(dev[0], dev[1], dev[2], dev[3], None, 0)
    res = run()
    out = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    Tg = np.array(res.transformation, np.float32).reshape(4, 4).T
    print("fast_global_registration 20000 + 20000 points, 33 dimensions, defaults   %8.3f ms (of 5: %.3f .. %.3f)   fitness %.4f, "
          "|T - T_gt|_F = %.3g" % (float(np.median(out)), min(out), max(out), res.fitness, np.linalg.norm(Tg - T)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
