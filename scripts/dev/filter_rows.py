#!/usr/bin/env python3
"""FarthestPointDownSample and GaussianFilter at scale, through the Engine on device memory: the fragment scan of
tests/golden (113,662 points) and a generated 10M-point cloud (1000 blobs plus 5 % noise, the cloud of iss_rows.py).
Per case the first call's and the median-of-5 host wall time, one JSON line each:

  fps_fragment / fps_blobs      1024 samples; with the time, the achieved bytes/s of the sample passes counted at
                                20 B per point per sample (12 B of the point, dist read and written) and its share of
                                the HBM peak
  gauss_fragment / gauss_blobs  max_nn = 50, a radius that holds about 50 points, sigma2 = (radius / 2)^2
  iss_fragment / iss_blobs      the yardstick of GaussianFilter: Engine.iss_keypoints at the same radius and capacity --
                                its pass 0 (iss_kernel<0, 64>) is the walk gaussian_kernel<64> does, adding nine
                                cumulants where the filter adds weights

Every case runs in a child process of its own under its own time limit, and the first failure ends the run.  Under
`rocprofv3 --kernel-trace --stats -- python scripts/dev/filter_rows.py --case NAME --once` the kernel table splits a call
into the tree's build kernels, fps_step / gaussian_kernel / iss_kernel and the gather.

    python scripts/dev/filter_rows.py [--case NAME] [--once] [--n N] [--samples K]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12            # bytes/s, MI355X
CASES = {"fps_fragment": 120, "fps_blobs": 300, "gauss_fragment": 120, "gauss_blobs": 300, "iss_fragment": 120, "iss_blobs": 300}
FRAGMENT_RADIUS, BLOBS_RADIUS = 0.03, 0.25


def blobs(n, seed=3):
    rng = np.random.default_rng(seed)
    k = n // 20
    centres = rng.uniform(-50, 50, (1000, 3))
    pts = np.concatenate([centres[rng.integers(0, 1000, n - k)] + rng.normal(0, 0.6, (n - k, 3)),
                          rng.uniform(-60, 60, (k, 3))]).astype(np.float32)
    return pts[rng.permutation(n)]


def one(a):
    import torch
    from cupoch_amd.engine import Engine
    eng = Engine(0)
    cloud = a.case.split("_")[1]
    if cloud == "fragment":
        pts = np.load(os.path.join(ROOT, "tests", "golden", "fragment_points.npz"))["points"].astype(np.float32)
        radius = FRAGMENT_RADIUS
    else:
        pts, radius = blobs(a.n), BLOBS_RADIUS
    pts = torch.from_numpy(pts).cuda()
    n = int(pts.shape[0])

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def timed(fn):
        r, first = wall(fn)
        rest = [] if a.once else [wall(fn)[1] for _ in range(5)]
        return r, round(first, 3), round(float(np.median(rest)), 3) if rest else None

    row = {"case": a.case, "points": n}
    if a.case.startswith("fps"):
        (_, _, _, idx), first, med = timed(lambda: eng.farthest_point_downsample(pts, a.samples))
        nbytes = 20.0 * n * (a.samples - 1)
        t = (med if med is not None else first) * 1e-3
        row.update(samples=a.samples, distinct=int(idx.unique().numel()), bytes_per_point_per_sample=20,
                   achieved_TB_per_s=round(nbytes / t / 1e12, 3), share_of_hbm_peak=round(nbytes / t / HBM_PEAK, 3))
    elif a.case.startswith("gauss"):
        (p, _, _), first, med = timed(lambda: eng.gaussian_filter(pts, radius, (radius / 2) ** 2, 50))
        row.update(radius=radius, max_nn=50, mean_shift=round(float((p - pts).norm(dim=1).mean()), 6))
    else:
        (_, m, _, _, _, cnt), first, med = timed(lambda: eng.iss_keypoints(pts, radius, radius * 2 / 3, max_neighbors=50, want_response=True))
        row.update(radius=radius, max_nn=50, keypoints=m, mean_row=round(float(cnt.float().mean()), 2),
                   rows_at_the_cap=round(float((cnt >= 50).float().mean()), 4))
    row.update(first_call_ms=first, median_of_5_ms=med)
    print(json.dumps(row), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if a.case:
        return one(a)
    for case, limit in CASES.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--n", str(a.n), "--samples", str(a.samples)] + (["--once"] if a.once else [])
        rc = subprocess.run(cmd, timeout=limit).returncode
        if rc != 0:
            sys.exit("%s ended with status %d: nothing further is started" % (case, rc))


if __name__ == "__main__":
    main()
