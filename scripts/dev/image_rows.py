"""Times of the image calls through the C ABI at 640x480 and 1280x960: the five named filters, the fused pyramid level
against Filter then Downsample as two calls, the bilateral filter at diameters 2, 5 and 15 with each exponential (the
hardware 2^x that mi_icp_image_bilateral runs, and expf), Transpose, and create_float_image from uint8 x 3.

A figure is a CALL time: device events around a batch of calls issued back to back on the engine's stream, divided by
the number of calls, the median of 5 batches after a warm-up batch -- launch gaps included, no wait inside.  The
engine wrappers allocate their outputs (torch's caching allocator: no device allocation in the timed window after the
warm-up).  Images of these sizes (1.2 and 4.9 MB) stay in the caches between calls, so the share of the HBM peak (8 TB/s)
on algorithmic bytes (one read and one write of the images) says how far a call is from the memory bound, not what the
memory delivered.  For the bilateral filter the rate is taps per second, (2 d + 1)^2 per pixel.

    python scripts/dev/image_rows.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12            # bytes/s, MI355X
F = np.float32


def call_ms(fn, calls, n=5):
    import torch
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return float(np.median(out))


def row(name, ms, nbytes, note=""):
    print("%-46s %8.4f ms   %6.3f TB/s = %5.1f %% of the HBM peak on %5.2f MB%s" %
          (name, ms, nbytes / (ms * 1e-3) / 1e12, 100.0 * nbytes / (ms * 1e-3) / HBM_PEAK, nbytes / 1e6, note), flush=True)


def main():
    import torch
    import image_exact as ix
    from cupoch_amd import geometry as g
    if not torch.cuda.is_available():
        raise SystemExit("image_rows.py needs a GPU: there is nothing to time without one")
    eng = g.get_engine()
    for w, h in ((640, 480), (1280, 960)):
        px = w * h
        size = "%dx%d" % (w, h)
        src = torch.from_numpy(ix.bilateral_image(w, h, 1)).cuda()
        calls = 200
        for kind, name in ((ix.GAUSSIAN3, "Gaussian3"), (ix.GAUSSIAN5, "Gaussian5"), (ix.GAUSSIAN7, "Gaussian7"),
                           (ix.SOBEL3DX, "Sobel3Dx"), (ix.SOBEL3DY, "Sobel3Dy")):
            dx, dy = ix.NAMED[kind]
            row("filter %s %s" % (name, size), call_ms(lambda: eng.image_filter(src, dx, dy), calls), 8.0 * px)
        row("pyramid level, fused %s" % size, call_ms(lambda: eng.image_pyramid_level(src), calls), 5.0 * px)
        g3 = ix.NAMED[ix.GAUSSIAN3]
        row("pyramid level, Filter then Downsample %s" % size,
            call_ms(lambda: eng.image_downsample(eng.image_filter(src, *g3)), calls), 13.0 * px, "  (two calls)")
        row("downsample float %s" % size, call_ms(lambda: eng.image_downsample(src), calls), 5.0 * px)
        for d in (2, 5, 15):
            taps = float((2 * d + 1) ** 2) * px
            for kind, name in ((1, "hardware 2^x"), (0, "expf")):
                ms = call_ms(lambda: eng.image_bilateral(src, d, 0.5, 3.0, exp_kind=kind), 200 if d < 15 else 20)
                row("bilateral d=%d %s %s" % (d, name, size), ms, 8.0 * px, "  %.1f G taps/s" % (taps / (ms * 1e-3) / 1e9))
        row("transpose float %s" % size, call_ms(lambda: eng.image_move(src, 0), calls), 8.0 * px)
        rgb = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
        row("transpose uint8 x 3 %s" % size, call_ms(lambda: eng.image_move(rgb, 0), calls), 6.0 * px)
        row("create_float_image from uint8 x 3 %s" % size, call_ms(lambda: eng.image_create_float(rgb, 1), calls), 7.0 * px)
        u16 = torch.from_numpy(np.random.default_rng(3).integers(0, 9000, (h, w)).astype(np.uint16)).cuda()
        row("convert_depth_to_float_image uint16 %s" % size, call_ms(lambda: eng.image_depth_to_float(u16, 1000.0, 3.0), calls), 6.0 * px)


if __name__ == "__main__":
    main()
