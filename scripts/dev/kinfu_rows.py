"""Times and poses of kinfu.KinfuPipeline on the five frames of tests/golden/rgbd, with the settings of
the reference's example (examples/python/advanced/kinfu.py): the default option with distance_threshold = 5.0, frames
made with create_from_color_and_depth(..., depth_trunc=4.0, convert_rgb_to_intensity=False), PrimeSense intrinsics.

    python scripts/dev/kinfu_rows.py [runs]
        (a) process_frame: the host clock around one call and a wait, frames 1-4 of `runs` (default 3) passes over the
            sequence, every figure listed and their median; the first frame of each pass; and where a frame's time
            goes -- measurement, pose estimation, integrate, model pyramid -- by device events around the same steps
            called by hand (kinfu.KinfuPipeline.process_frame is those calls).
        (b) the model pyramid: volume.raycast_levels with 4 levels against four volume.raycast calls, alternating in
            one process, 7 pairs, host clock around call and wait; medians and the spread of each.
        (c) tracking: cur_pose after frame k against inv(pose_0) . pose_k of tests/golden/rgbd/odometry.log.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kinfu -- python scripts/dev/kinfu_rows.py --frames
        runs the five frames once and nothing else, for the kernel trace.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
RGBD = os.path.join(ROOT, "tests", "golden", "rgbd")
F = np.float32


def load():
    """-> ([RGBDImage on the device], [pose of the log, relative to frame 0])"""
    from PIL import Image
    from cupoch_amd import geometry as g
    lines = open(os.path.join(RGBD, "odometry.log")).read().split("\n")
    frames, poses = [], []
    k = 0
    while k * 5 + 4 < len(lines) and lines[k * 5].strip():
        poses.append(np.array([[float(x) for x in lines[k * 5 + 1 + r].split()] for r in range(4)], np.float64))
        depth = np.asarray(Image.open(os.path.join(RGBD, "depth", "%05d.png" % k))).astype(np.uint16)
        color = np.ascontiguousarray(np.asarray(Image.open(os.path.join(RGBD, "color", "%05d.jpg" % k)).convert("RGB")))
        frames.append(g.RGBDImage.create_from_color_and_depth(color, depth, depth_trunc=4.0, convert_rgb_to_intensity=False))
        k += 1
    return frames, [np.linalg.inv(poses[0]) @ p for p in poses]


def pipeline():
    from cupoch_amd import camera, kinfu
    opt = kinfu.KinfuOption()
    opt.distance_threshold = 5.0
    return kinfu.KinfuPipeline(camera.PinholeCameraIntrinsic(640, 480, 525.0, 525.0, 319.5, 239.5), opt)


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(v):
    return " ".join("%.2f" % x for x in v)


def stages(pipe, image):
    """one frame by hand, as process_frame does it, with device events between the steps -> ms per step"""
    import torch
    from cupoch_amd import kinfu
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    o = pipe.option
    ev[0].record()
    _, smooth, clouds = pipe.surface_measurement(image)
    ev[1].record()
    E = kinfu.inverse_transform(pipe.cur_pose)
    if pipe.frame_id > 0:
        E, _ = kinfu.pose_estimation(o, E, pipe.model_pyramid, clouds)
        pipe.cur_pose = kinfu.inverse_transform(E)
    ev[2].record()
    assert pipe.volume.integrate(smooth[0], pipe.intrinsic, E)
    ev[3].record()
    pipe.model_pyramid = pipe.volume.raycast_levels(pipe.intrinsic, E, o.sdf_trunc, o.num_pyramid_levels)
    ev[4].record()
    ev[4].synchronize()
    pipe.frame_id += 1
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]


def main():
    import torch
    from cupoch_amd import kinfu
    if not torch.cuda.is_available():
        raise SystemExit("kinfu_rows.py needs a GPU: there is nothing to time without one")
    frames, truth = load()
    pipe = pipeline()
    if len(sys.argv) > 1 and sys.argv[1] == "--frames":
        for f in frames:
            assert pipe.process_frame(f)
        torch.cuda.synchronize()
        return
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    later, first = [], []
    for r in range(runs):
        pipe.reset()
        for k, f in enumerate(frames):
            ms, ok = wall_ms(lambda: pipe.process_frame(f))
            assert ok
            (first if k == 0 else later).append(ms)
    print("(a) process_frame 640x480, volume 512^3, 4 levels: frames 1-4 median %.2f ms   every run: %s" % (np.median(later), fmt(later)))
    print("    the first frame (no pose estimation): %s ms; the very first also loads the code objects and sizes the buffers" % fmt(first))
    pipe.reset()
    rows = [stages(pipe, f) for f in frames]
    for name, col in zip(("measurement", "pose estimation", "integrate", "model pyramid"), zip(*rows)):
        print("    %-16s frames 1-4 median %7.3f ms   frame 0 %7.3f   every frame: %s" % (name, np.median(col[1:]), col[0], fmt(col)))

    # (c) before anything else moves the pose
    print("(c) cur_pose against inv(pose_0) . pose_k of the log:")
    pipe.reset()
    for k, f in enumerate(frames):
        assert pipe.process_frame(f)
        T = np.asarray(pipe.cur_pose, np.float64)
        dR = truth[k][:3, :3].T @ T[:3, :3]
        ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
        print("    frame %d: translation error %.4f m (the log moved %.4f m), rotation error %.3f deg" %
              (k, np.linalg.norm(T[:3, 3] - truth[k][:3, 3]), np.linalg.norm(truth[k][:3, 3]), ang))

    # (b) on the volume of the five frames, from the last pose
    E, o, K = kinfu.inverse_transform(pipe.cur_pose), pipe.option, pipe.intrinsic
    one = lambda: pipe.volume.raycast_levels(K, E, o.sdf_trunc, 4)
    four = lambda: [pipe.volume.raycast(K.create_pyramid_level(i), E, o.sdf_trunc) for i in range(4)]
    one(), four()
    t_one, t_four = [], []
    for _ in range(7):
        t_one.append(wall_ms(one)[0])
        t_four.append(wall_ms(four)[0])
    sizes = [len(c.points) for c in one()]
    print("(b) model pyramid, 4 levels (%s points): raycast_levels median %.3f ms [%.3f .. %.3f]   four raycast calls median %.3f ms [%.3f .. %.3f]" %
          (" ".join(map(str, sizes)), np.median(t_one), min(t_one), max(t_one), np.median(t_four), min(t_four), max(t_four)))
    print("    pairs, alternating (levels / four): %s" % "  ".join("%.3f/%.3f" % p for p in zip(t_one, t_four)))


if __name__ == "__main__":
    main()
