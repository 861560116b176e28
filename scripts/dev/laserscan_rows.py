"""Times of geometry.LaserScanBuffer's conversions and filters through the C ABI, each the median of 5 after a warm-up
call (host wall time around the calls and a device synchronise), and next to each the share of the HBM peak (8 TB/s) on
algorithmic bytes -- for from_points the 12 bytes read per point.  A from_points sample is 12 calls over three copies of
the cloud in turn (360 MB: more than the 256 MiB Infinity Cache, so that no call finds its input there), divided by 12;
the small rows are single calls and measure launch and wait overheads as much as the kernels:
  from_points of 10M uniform points into 1081x1 and 1081x16 bins (LDS path), into the smallest grid above the LDS limit
  (global path), and of 10M points sorted by angle (the worst contention per bin) on both paths;
  to_points of 50 scans x 1081 steps; from_depth of a 640x480 frame; the shadow filter on 50 x 1081 with window 5.

    python scripts/dev/laserscan_rows.py [points]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12            # bytes/s, MI355X
F = np.float32


def median_ms(fn, sync, n=5, calls=1):
    fn()
    sync()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.median(out))


def row(name, ms, nbytes, note=""):
    print("%-44s %8.3f ms   %7.3f TB/s = %5.1f %% of the HBM peak on %.1f MB%s" %
          (name, ms, nbytes / (ms * 1e-3) / 1e12, 100.0 * nbytes / (ms * 1e-3) / HBM_PEAK, nbytes / 1e6, note), flush=True)


def main():
    import torch
    import tsdf_exact as tx
    from cupoch_amd import geometry
    eng = geometry.get_engine()
    sync = torch.cuda.synchronize
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    lds_max, _ = eng.laserscan_limits()
    rng = np.random.default_rng(0)
    ang = rng.uniform(-np.pi, np.pi, n)
    r = rng.uniform(0.5, 30.0, n)
    pts = np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(0.0, 2.0, n)], 1).astype(F)
    uniform = [torch.from_numpy(pts).cuda() for _ in range(3)]
    by_angle = [torch.from_numpy(pts[np.argsort(ang)]).cuda() for _ in range(3)]
    inc = float(F(2 * np.pi) / F(1080.5))
    div_global = lds_max // 1081 + 1
    for name, clouds, div in (("uniform", uniform, 1), ("uniform", uniform, 16), ("uniform", uniform, div_global),
                             ("sorted by angle", by_angle, 1), ("sorted by angle", by_angle, 16),
                             ("sorted by angle", by_angle, div_global)):
        path = []
        ms = median_ms(lambda: path.append(eng.laserscan_from_points(clouds[len(path) % 3], inc, 0.0, 2.0, div, 0.1, 40.0)[1]),
                       sync, calls=12)
        row("from_points %dM %s 1081x%d (%s)" % (n // 1_000_000, name, div, "LDS" if path[-1] == 0 else "global"), ms, 12.0 * n)

    steps, scans = 1081, 50
    buf = geometry.LaserScanBuffer(steps, scans)
    for k in range(scans):
        buf.add_ranges(torch.from_numpy(rng.uniform(0.5, 30.0, steps).astype(F)).cuda(),
                       np.eye(4, dtype=F), torch.from_numpy(rng.random(steps).astype(F)).cuda())
    ms = median_ms(lambda: geometry.PointCloud.create_from_laserscanbuffer(buf, 0.1, 40.0), sync)
    row("to_points 50 x 1081 (with intensities)", ms, scans * steps * (8 + 24), "  (one wait for the count inside)")
    ms = median_ms(lambda: buf.scan_shadow_filter(0.17, 2.97, 5, 1, False), sync)
    row("shadow filter 50 x 1081, window 5", ms, scans * steps * 8, "  (one wait inside)")
    ms = median_ms(lambda: buf.range_filter(1.0, 20.0), sync)
    row("range filter 50 x 1081", ms, scans * steps * 8)

    W, H, fx, fy, cx, cy = tx.PRIMESENSE
    E = np.eye(4, dtype=F)
    depth, _ = tx.render_scene(W, H, fx, fy, cx, cy, E, [((0.0, 0.0, 1.0), 3.0)], ((0.2, 0.1, 2.0), 0.5), holes=True)
    d = torch.from_numpy(depth).cuda()
    ms = median_ms(lambda: eng.laserscan_from_depth(d, (fx, fy, cx, cy), 0.005, -1.5, 1.5, 1, 0.1, 10.0), sync)
    row("from_depth %dx%d float32" % (W, H), ms, W * H * 4)


if __name__ == "__main__":
    main()
