#!/usr/bin/env python3
"""SegmentPlane at scale: a 10M-point cloud (a tilted slab, sigma 0.004, with 30 % uniform clutter, shuffled) through
Engine.segment_plane(0.02, 3, num_iterations) on device memory at num_iterations = 1, 100 and 1000, and the fragment
scan of tests/golden at 1000: per case the first call's and the median-of-5 host wall time, one JSON line each.  Under
`rocprofv3 --kernel-trace --stats` (with --once: one call per case) the kernel table splits a call into the hypotheses
(seg_hypotheses), the scoring pass (seg_score), the selection (seg_select / seg_tie_partial / seg_pick), the inlier list
(seg_flags, the scan, seg_list) and the refit (seg_centroid_* / seg_moments_partial / seg_refit_final).

    python scripts/dev/segment_plane_rows.py [--once] [--n N] [--iterations 1,100,1000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def cloud(n, seed=3, clutter=0.3):
    rng = np.random.default_rng(seed)
    k = int(n * clutter)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    slab = np.column_stack([rng.uniform(-4, 4, (n - k, 2)), rng.normal(0, 0.004, n - k)]) @ q.T
    pts = np.concatenate([slab, rng.uniform(-4, 4, (k, 3))]).astype(np.float32)
    return pts[rng.permutation(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--iterations", default="1,100,1000")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from cupoch_amd.engine import Engine
    eng = Engine(0)
    frag = np.load(os.path.join(ROOT, "tests", "golden", "fragment_points.npz"))["points"].astype(np.float32)
    cases = [("slab", torch.from_numpy(cloud(a.n)).cuda(), int(k)) for k in a.iterations.split(",")]
    cases.append(("fragment", torch.from_numpy(frag).cuda(), 1000))
    for name, pts, iters in cases:
        def wall():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = eng.segment_plane(pts, 0.02, 3, iters, 1)
            torch.cuda.synchronize()
            return r, (time.perf_counter() - t0) * 1e3
        (plane, idx, ransac, best, count), first = wall()
        rest = [] if a.once else [wall()[1] for _ in range(5)]
        print(json.dumps({"call": "segment_plane", "cloud": name, "points": int(pts.shape[0]), "num_iterations": iters,
                          "winner": best, "inliers": count, "plane": [round(float(v), 5) for v in plane],
                          "first_call_ms": round(first, 3),
                          "median_of_5_ms": round(float(np.median(rest)), 3) if rest else None}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
