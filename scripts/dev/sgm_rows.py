"""Times of imageproc.SemiGlobalMatching and PointCloud.create_from_disparity at 640x480.

    python scripts/dev/sgm_rows.py
        call times: one ProcessFrame at D = 128, 64 and 256 with ScanPath8 and at D = 128 with ScanPath4 (defaults
        otherwise), and one create_from_disparity.  A figure is device events around ONE call on the engine's stream
        (images already on the device), the median of 5 after a warm-up call; the first call of a fresh object in a
        fresh process -- code objects loaded, the workspace allocated -- is timed by the host clock around
        construction, call and a wait, and stated separately.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sgm -- python scripts/dev/sgm_rows.py --frames 20 128 8
        runs 20 frames and nothing else, for the kernel trace;
    python scripts/dev/sgm_rows.py --stats DIR/.../sgm_kernel_stats.csv 128 8
        then prints the per-kernel rows: average time, the bytes the kernel must move (from the shapes) and their
        share of the HBM peak, and for the path kernel the steps of its serial chain.
"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12            # bytes/s, MI355X
W, H = 640, 480


def option(disp_size, paths):
    from cupoch_amd import imageproc as ip
    return ip.SGMOption(W, H, disp_size=ip.DisparitySizeType(disp_size), path_type=ip.PathType.ScanPath8 if paths == 8 else ip.PathType.ScanPath4)


def frames():
    import torch
    import sgm_exact as sx
    from cupoch_amd import geometry as g
    left, right, _ = sx.pair(W, H, 3)
    return g.Image(torch.from_numpy(left).cuda()), g.Image(torch.from_numpy(right).cuda())


def one_call_ms(fn, n=5):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), out


def kernel_bytes(disp_size, paths):
    """the bytes each kernel must read and write, from the shapes"""
    px = W * H
    vol = px * disp_size
    return {"sgm_census": 2 * px * (1 + 4), "sgm_paths": paths * vol + paths * 2 * px * 4, "sgm_wta": paths * vol + px * (2 + 4),
            "sgm_tail": px * (2 + 4 + 1), "disparity_points": px * (1 + 3 + 24)}


def stats(path, disp_size, paths):
    want = kernel_bytes(disp_size, paths)
    with open(path) as f:
        rows = list(csv.DictReader(f))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        key = next((k for k in want if k in name), None)
        if key is None:
            continue
        avg_ns = float(r.get("AverageNs") or r.get("Average") or 0.0)
        ms = avg_ns * 1e-6
        nbytes = want[key]
        note = ""
        if key == "sgm_paths":
            note = "   %.0f ns a step of the longest chain (%d pixels)" % (avg_ns / W, W)
        print("%-18s calls %4s  %8.4f ms   %6.1f MB -> %5.2f TB/s = %4.1f %% of the HBM peak%s" %
              (key, r.get("Calls", "?"), ms, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e12, 100.0 * nbytes / (ms * 1e-3) / HBM_PEAK, note))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--stats":
        return stats(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    import torch
    from cupoch_amd import camera, geometry as g, imageproc as ip
    if not torch.cuda.is_available():
        raise SystemExit("sgm_rows.py needs a GPU: there is nothing to time without one")
    left, right = frames()
    if len(sys.argv) > 1 and sys.argv[1] == "--frames":
        m = ip.SemiGlobalMatching(option(int(sys.argv[3]), int(sys.argv[4])))
        for _ in range(int(sys.argv[2])):
            m.process_frame(left, right)
        torch.cuda.synchronize()
        return
    torch.cuda.synchronize()
    first = None
    for disp_size, paths in ((128, 8), (64, 8), (256, 8), (128, 4)):
        t0 = time.perf_counter()
        m = ip.SemiGlobalMatching(option(disp_size, paths))
        out = m.process_frame(left, right)
        torch.cuda.synchronize()
        cold = (time.perf_counter() - t0) * 1e3
        first = cold if first is None else first
        ms, all_ms = one_call_ms(lambda: m.process_frame(left, right))
        valid = float((out.data != 255).float().mean())
        print("ProcessFrame %dx%d D=%3d ScanPath%d  %7.3f ms (median of 5: %s)   object made + first call %7.1f ms   valid %.3f" %
              (W, H, disp_size, paths, ms, " ".join("%.3f" % v for v in all_ms), cold, valid), flush=True)
        del m
    print("the very first of those, with the code objects to load: %.1f ms" % first)
    disp = ip.SemiGlobalMatching(option(128, 8)).process_frame(left, right)
    color = g.Image(torch.from_numpy(np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda())
    k = camera.PinholeCameraIntrinsic(W, H, 525.0, 525.0, 319.5, 239.5)
    ms, all_ms = one_call_ms(lambda: g.PointCloud.create_from_disparity(disp, color, k, k, 0.12))
    print("create_from_disparity %dx%d  %7.4f ms (median of 5: %s)" % (W, H, ms, " ".join("%.4f" % v for v in all_ms)))


if __name__ == "__main__":
    main()
