#!/usr/bin/env python3
"""ClusterDBSCAN at scale: a 10M-point cloud (1000 Gaussian blobs, sigma 0.6, plus 5 % uniform noise, shuffled) through
Engine.cluster_dbscan(eps = 0.19, min_points = 10) on device memory: the whole call's first and median-of-5 host wall
time, one JSON line.  Under `rocprofv3 --kernel-trace --stats` (with --once: one call) the kernel table splits the call
into the tree build, the rows (knn_normals_kernel<4>), the graph (dbscan_init / hook / flatten / classify / round /
step) and the labels (dbscan_starts, the scan, dbscan_labels).

    python scripts/dev/dbscan_rows.py [--once] [--n N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def cloud(n, seed=3):
    rng = np.random.default_rng(seed)
    nb = max(1, n // 10_000)
    centres = rng.uniform(-50, 50, (nb, 3)) * (nb / 200.0) ** (1.0 / 3.0)
    k = n - n // 20
    pts = np.concatenate([centres[rng.integers(0, nb, k)] + rng.normal(0, 0.6, (k, 3)),
                          rng.uniform(-60, 60, (n - k, 3)) * (nb / 200.0) ** (1.0 / 3.0)]).astype(np.float32)
    return pts[rng.permutation(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--eps", type=float, default=0.19)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from cupoch_amd.engine import Engine
    pts = torch.from_numpy(cloud(a.n)).cuda()
    eng = Engine(0)

    def wall():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.cluster_dbscan(pts, a.eps, 10)
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3
    (lab, deg, nc), first = wall()
    rest = [] if a.once else [wall()[1] for _ in range(5)]
    lab, deg = lab.cpu().numpy(), deg.cpu().numpy()
    print(json.dumps({"call": "cluster_dbscan", "points": a.n, "eps": a.eps, "min_points": 10,
                      "mean_degree": round(float(deg.mean()), 2), "max_degree": int(deg.max()),
                      "clusters": nc, "noise": int((lab < 0).sum()), "first_call_ms": round(first, 2),
                      "median_of_5_ms": round(float(np.median(rest)), 2) if rest else None}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
