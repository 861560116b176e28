"""Times of integration::ScalableTSDFVolume for the 640x480 frame of scripts/dev/tsdf_rows.py (voxel 8/512, sdf_trunc
0.05, the same camera, wall and sphere), each the median of 5 after a warm-up call: the first frame's Integrate (every
unit opens), a steady-state Integrate (no new unit), ExtractPointCloud and ExtractVoxelPointCloud, for NoColor and RGB8;
and in the same run, as the yardstick, UniformTSDFVolume.integrate and extract_point_cloud at 512^3.  Prints one line
per row with the units open, the voxels projected (units x 4096, or resolution^3) and updated, and the floor the
updated voxels imply (voxels x bytes per voxel x 2 at 8 TB/s).

    python scripts/dev/scalable_tsdf_rows.py            every step, each in a child process under its own time limit
    python scripts/dev/scalable_tsdf_rows.py STEP       one of: scalable-nocolor scalable-rgb8 uniform-nocolor uniform-rgb8
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = {"scalable-nocolor": 120, "scalable-rgb8": 120, "uniform-nocolor": 120, "uniform-rgb8": 120}   # seconds each
VOXEL, TRUNC, RES = 8.0 / 512.0, 0.05, 512


def median_ms(fn, sync, n=5, before=None):
    out = []
    for k in range(n + 1):                 # the first call is the warm-up
        if before:
            before()
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out[1:]))


def scene():
    import tsdf_exact as tx
    from cupoch_amd import camera
    W, H, fx, fy, cx, cy = tx.PRIMESENSE
    E = np.eye(4, dtype=np.float32)
    E[:3, 3] = (-2.0, -2.0, 0.5)
    depth, color = tx.render_scene(W, H, fx, fy, cx, cy, E, [((0.0, 0.0, 1.0), 2.0)], ((2.2, 2.1, 1.4), 0.5), holes=True)
    return camera.PinholeCameraIntrinsic(W, H, fx, fy, cx, cy), E, depth, color


def floor_ms(updated, ct):
    return updated * (8 if ct == 0 else 20) * 2 / 8e12 * 1e3


def run(step):
    import torch
    from cupoch_amd import geometry, integration, integration_scalable
    kind, name = step.split("-")
    ct = 0 if name == "nocolor" else 1
    K, E, depth, color = scene()
    sync = torch.cuda.synchronize
    img = geometry.RGBDImage(None if ct == 0 else torch.from_numpy(color).cuda(), torch.from_numpy(depth).cuda())
    T = integration.TSDFVolumeColorType(ct)
    if kind == "uniform":
        vol = integration.UniformTSDFVolume(VOXEL * RES, RES, TRUNC, T)
        ms = median_ms(lambda: vol.integrate(img, K, E), sync)
        _, w, _ = vol._eng.tsdf_get_voxels(vol._vol, vol.voxel_num, False, on_device=True)
        updated = int((w > 0).sum().item())
        del w
        print("uniform  %-7s integrate                 %8.3f ms   %d voxels projected, %d updated, floor %.4f ms" %
              (name, ms, RES ** 3, updated, floor_ms(updated, ct)), flush=True)
        ms = median_ms(vol.extract_point_cloud, sync)
        print("uniform  %-7s extract_point_cloud       %8.3f ms   %d points" % (name, ms, len(vol.extract_point_cloud().points)),
              flush=True)
        return
    vol = integration_scalable.ScalableTSDFVolume(VOXEL, TRUNC, T)
    ms_first = median_ms(lambda: vol.integrate(img, K, E), sync, before=vol.reset)
    vol.reset()
    vol.integrate(img, K, E)
    units = vol.num_volume_units()[0]
    _, _, w, _ = vol._eng.stsdf_get_units(vol._vol, False, on_device=True)
    updated = int((w > 0).sum().item())
    tail = "%d units, %d voxels projected, %d updated, floor %.4f ms" % (units, units * 4096, updated, floor_ms(updated, ct))
    print("scalable %-7s integrate, first frame    %8.3f ms   %s" % (name, ms_first, tail), flush=True)
    ms = median_ms(lambda: vol.integrate(img, K, E), sync)
    assert vol.num_volume_units()[0] == units
    print("scalable %-7s integrate, steady state   %8.3f ms   %s" % (name, ms, tail), flush=True)
    ms = median_ms(vol.extract_point_cloud, sync)
    print("scalable %-7s extract_point_cloud       %8.3f ms   %d points" % (name, ms, len(vol.extract_point_cloud().points)),
          flush=True)
    ms = median_ms(vol.extract_voxel_point_cloud, sync)
    print("scalable %-7s extract_voxel_point_cloud %8.3f ms   %d points" %
          (name, ms, len(vol.extract_voxel_point_cloud().points)), flush=True)


def main():
    if len(sys.argv) > 1:
        return run(sys.argv[1])
    for step, limit in STEPS.items():      # a fresh child per step; the first that fails or overruns ends the run
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), step], timeout=limit).returncode
        if rc != 0:
            sys.exit("step %s ended with status %d" % (step, rc))


if __name__ == "__main__":
    main()
