"""Times of integration::UniformTSDFVolume for a 640x480 frame, each the median of 5 after a warm-up call:
Integrate on a 512^3 volume (NoColor and RGB8) with a camera that sees about a tenth of the volume, Raycast at the four
pyramid levels, and both extractions.  Prints one line per row, with the updated-voxel count and the floor it implies
(updated voxels x bytes per voxel x 2 at 8 TB/s) for Integrate.

    python scripts/dev/tsdf_rows.py [resolution]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, sync, n=5):
    fn()
    sync()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    import torch
    import tsdf_exact as tx
    from cupoch_amd import camera, geometry, integration
    res = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    W, H, fx, fy, cx, cy = tx.PRIMESENSE
    K = camera.PinholeCameraIntrinsic(W, H, fx, fy, cx, cy)
    length, trunc = 8.0, 0.05
    # a camera in the volume's positive octant looking along +z at a wall 2.5 m away: its frustum holds about a
    # tenth of the volume's voxels
    E = np.eye(4, dtype=np.float32)
    E[:3, 3] = (-2.0, -2.0, 0.5)
    depth, color = tx.render_scene(W, H, fx, fy, cx, cy, E, [((0.0, 0.0, 1.0), 2.0)], ((2.2, 2.1, 1.4), 0.5), holes=True)
    sync = torch.cuda.synchronize
    for name, ct in (("NoColor", 0), ("RGB8", 1)):
        vol = integration.UniformTSDFVolume(length, res, trunc, integration.TSDFVolumeColorType(ct))
        img = geometry.RGBDImage(None if ct == 0 else torch.from_numpy(color).cuda(), torch.from_numpy(depth).cuda())
        ms = median_ms(lambda: vol.integrate(img, K, E), sync)
        t, w, _ = vol._eng.tsdf_get_voxels(vol._vol, vol.voxel_num, False, on_device=True)
        updated = int((w > 0).sum().item())
        bytes_per = 8 if ct == 0 else 20
        print("integrate %d^3 %-7s %8.3f ms   %d voxels updated per frame, floor %.4f ms" %
              (res, name, ms, updated, updated * bytes_per * 2 / 8e12 * 1e3), flush=True)
        if ct == 1:
            for level in range(4):
                Kl = K.create_pyramid_level(level)
                ms = median_ms(lambda: vol.raycast(Kl, E, trunc), sync)
                print("raycast level %d (%dx%d) %8.3f ms   %d points" %
                      (level, Kl.width, Kl.height, ms, len(vol.raycast(Kl, E, trunc).points)), flush=True)
            ms = median_ms(vol.extract_point_cloud, sync)
            print("extract_point_cloud       %8.3f ms   %d points" % (ms, len(vol.extract_point_cloud().points)), flush=True)
            ms = median_ms(vol.extract_voxel_point_cloud, sync)
            print("extract_voxel_point_cloud %8.3f ms   %d points" % (ms, len(vol.extract_voxel_point_cloud().points)), flush=True)
        del vol


if __name__ == "__main__":
    main()
