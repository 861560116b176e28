#!/usr/bin/env python3
"""ComputeISSKeypoints at scale: the fragment scan of tests/golden with the default arguments (both radii from the
model resolution) and a generated 10M-point cloud (1000 blobs plus 5 % noise, the cloud of dbscan_rows.py) at a salient
radius that holds about 100 points, through Engine.iss_keypoints on device memory: per case the first call's and the
median-of-5 host wall time, one JSON line each.  For the yardstick the same 10M cloud goes through
Engine.cluster_dbscan at the salient radius with max_edges = 100: its radius-row pass (knn_normals_kernel<4, 104>) is the
walk pass A does, writing rows where pass A writes 4 to 16 bytes per point.  Under `rocprofv3 --kernel-trace --stats`
(with --once: one call per case; counters in a run of their own) the kernel table splits a call into the tree (the
build kernels), the resolution pass (knn_normals_kernel<2, 32>, outlier_stats_partial, iss_resolution_sum), pass A
(iss_kernel<0, ...>), pass B (iss_kernel<1, ...>) and the count (the scan kernels).

    python scripts/dev/iss_rows.py [--once] [--n N] [--radius R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def blobs(n, seed=3):
    rng = np.random.default_rng(seed)
    k = n // 20
    centres = rng.uniform(-50, 50, (1000, 3))
    pts = np.concatenate([centres[rng.integers(0, 1000, n - k)] + rng.normal(0, 0.6, (n - k, 3)),
                          rng.uniform(-60, 60, (k, 3))]).astype(np.float32)
    return pts[rng.permutation(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--radius", type=float, default=0.3, help="salient radius of the generated cloud (non-maximum: 2/3 of it)")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from cupoch_amd.engine import Engine
    eng = Engine(0)
    frag = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "fragment_points.npz"))["points"].astype(np.float32)).cuda()
    big = torch.from_numpy(blobs(a.n)).cuda()

    def timed(fn):
        def wall():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return r, (time.perf_counter() - t0) * 1e3
        r, first = wall()
        rest = [] if a.once else [wall()[1] for _ in range(5)]
        return r, round(first, 3), round(float(np.median(rest)), 3) if rest else None

    for name, pts, kw in (("fragment", frag, {}), ("blobs", big, dict(salient_radius=a.radius, non_max_radius=a.radius * 2 / 3))):
        (mask, m, radii, sal, eig, cnt), first, med = timed(lambda: eng.iss_keypoints(pts, want_response=True, **kw))
        print(json.dumps({"call": "iss_keypoints", "cloud": name, "points": int(pts.shape[0]), "radii": [round(r, 6) for r in radii],
                          "keypoints": m, "mean_salient_row": round(float(cnt.float().mean()), 2),
                          "rows_at_the_cap": round(float((cnt >= 100).float().mean()), 4),
                          "pass_the_gates": round(float((sal >= 0).float().mean()), 4),
                          "first_call_ms": first, "median_of_5_ms": med}), flush=True)
    (lab, deg, nc), first, med = timed(lambda: eng.cluster_dbscan(big, a.radius, 10, 100))
    print(json.dumps({"call": "cluster_dbscan", "cloud": "blobs", "points": int(big.shape[0]), "eps": a.radius,
                      "mean_degree": round(float(deg.float().mean()), 2), "clusters": nc,
                      "first_call_ms": first, "median_of_5_ms": med}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
