"""kinfu.KinfuPipeline (the Python mirror) on the GPU against the same steps called by hand through the mirror's public
pieces (tests/kinfu_scene.py HandLoop: create_pyramid, bilateral_filter_pyramid_depth, point_cloud_pyramid,
pose_estimation, integrate, one raycast per level): 64 x 48 frames, a volume of resolution 64, 3 levels, a camera that
moves by about one voxel length and 0.01 rad per frame.

Measured on an MI355X (the tests print them): two runs of the hand-composed loop agree bit for bit and
the pipeline's poses equal theirs; after four moves (true motion 0.1844 Frobenius) the pose error is 0.0283 for both."""
import numpy as np
import pytest

import kinfu_scene as ks

pytestmark = pytest.mark.gpu
F = np.float32
FRAMES = 5                      # frame 0 and four moves


@pytest.fixture(scope="module")
def run():
    """the pipeline and the hand-composed loop (twice: is it deterministic?) over the same frames, with what the
    tests compare recorded on the way"""
    from cupoch_amd import kinfu
    K = ks.intrinsic()
    frames = [ks.rgbd(*ks.render(k)) for k in range(FRAMES)]
    pipe = kinfu.KinfuPipeline(K, ks.option())
    hands = [ks.HandLoop(K, ks.option()) for _ in range(2)]
    rec = {"pipe_pose": [], "hand_pose": [[], []], "measure_same": [], "frame_id": [], "ok": []}
    for k, image in enumerate(frames):
        clouds = [h.process(image) for h in hands]
        measured = pipe.surface_measurement(image)[2]               # does not depend on the pose: before or after
        rec["ok"].append(pipe.process_frame(image))
        rec["measure_same"].append(len(measured) == ks.LEVELS and all(ks.same_cloud(a, b) for a, b in zip(measured, clouds[0])))
        rec["pipe_pose"].append(np.array(pipe.cur_pose, F))
        rec["frame_id"].append(pipe.frame_id)
        for h, poses in zip(hands, rec["hand_pose"]):
            poses.append(h.pose.copy())
        if k == 0:
            rec["voxels0"] = (pipe.volume.get_voxels(), hands[0].volume.get_voxels())
            rec["model0"] = (list(pipe.model_pyramid), list(hands[0].model))
    rec["pipe"], rec["frames"], rec["K"] = pipe, frames, K
    return rec


def test_frame_0_equals_the_steps_by_hand(run):
    assert run["ok"][0] is True and run["frame_id"][0] == 1
    assert np.array_equal(run["pipe_pose"][0], np.eye(4, dtype=F))
    got, want = run["voxels0"]
    assert want[1].any() and ks.same(got[0], want[0]) and ks.same(got[1], want[1]) and ks.same(got[2], want[2])
    model, by_hand = run["model0"]
    assert len(model) == ks.LEVELS
    for i, (a, b) in enumerate(zip(model, by_hand)):
        assert len(b.points) > (60, 250, 1000)[2 - i] and ks.same_cloud(a, b), "level %d" % i


def test_measurement_pyramid_every_frame(run):
    assert run["measure_same"] == [True] * FRAMES


def test_frame_1_pose_is_the_hand_composed_one(run):
    """within 1e-5 Frobenius, the bound the project holds final transforms to; where two runs of the hand-composed loop
    agree bit for bit (they did on every run so far), bit equality is asserted instead"""
    assert run["ok"][1] is True and run["frame_id"][1] == 2
    a, b = run["hand_pose"][0][1], run["hand_pose"][1][1]
    got = run["pipe_pose"][1]
    print("frame 1: |pipeline - by hand|_F = %.3g, the two runs by hand %s" % (
        np.linalg.norm(got.astype(np.float64) - a), "agree bit for bit" if ks.same(a, b) else "differ"))
    assert not np.array_equal(got, np.eye(4, dtype=F))
    if ks.same(a, b):
        assert ks.same(got, a)
    else:
        assert np.linalg.norm(got.astype(np.float64) - a) <= 1e-5


def test_tracking(run):
    """The final pose error against the truth is at most that of the hand-composed loop on the same frames plus 1e-4
    (ten times the per-call transform bound of 1e-5, for four frames of accumulation); the true motion is at least
    100 times that margin, so a pipeline that stays at the identity fails."""
    truth = ks.true_pose(FRAMES - 1)[0]
    motion = ks.pose_error(np.eye(4), truth)
    e_pipe = ks.pose_error(run["pipe_pose"][-1], truth)
    e_hand = ks.pose_error(run["hand_pose"][0][-1], truth)
    print("tracking over %d frames: true motion %.4f, pipeline error %.3g, by hand %.3g" % (FRAMES, motion, e_pipe, e_hand))
    assert run["ok"] == [True] * FRAMES and run["frame_id"][-1] == FRAMES
    assert motion >= 100 * 1e-4
    assert e_pipe <= e_hand + 1e-4
    assert e_pipe < 0.5 * motion                                     # and it did track


def state(pipe):
    return pipe.volume.get_voxels(), np.array(pipe.cur_pose, F), pipe.frame_id, list(pipe.model_pyramid)


def unchanged(pipe, before):
    (v0, p0, f0, m0), (v1, p1, f1, m1) = before, state(pipe)
    return all(ks.same(a, b) for a, b in zip(v0, v1)) and ks.same(p0, p1) and f0 == f1 and \
        len(m0) == len(m1) and all(a is b for a, b in zip(m0, m1))


def test_refusals_and_reset(run, capsys):
    from cupoch_amd import geometry, kinfu, registration
    K, frames = run["K"], run["frames"]
    pipe = kinfu.KinfuPipeline(K, ks.option())
    assert pipe.process_frame(frames[0]) and pipe.process_frame(frames[1])
    before = state(pipe)
    d, c = ks.render(2)
    line = "[cupoch_amd] Error: [KinfuPipeline::ProcessFrame] "

    def refused(image, why):
        capsys.readouterr()
        assert pipe.process_frame(image) is False, why
        assert line + why in capsys.readouterr().out, why
        assert unchanged(pipe, before), why

    refused(geometry.RGBDImage(None, d), "The frame has no colour or no depth data.")
    refused(geometry.RGBDImage(c, None), "The frame has no colour or no depth data.")
    for levels in (0, 17):
        pipe.option.num_pyramid_levels = levels
        refused(frames[2], "num_pyramid_levels must be in [1, 16].")
    pipe.option.num_pyramid_levels = ks.LEVELS
    pipe.option.icp_iterations = [10, 10]
    refused(frames[2], "icp_iterations has fewer entries than num_pyramid_levels.")
    pipe.option.icp_iterations = [10, 10, 10]
    refused(geometry.RGBDImage(c[:24, :32].copy(), d[:24, :32].copy()), "The frame's size is not the intrinsic's.")
    refused(geometry.RGBDImage(c, (d * 1000).astype(np.uint16)), "Unsupported image format.")       # no pyramid of it
    refused(geometry.RGBDImage(np.ascontiguousarray(c[..., 0].astype(F) / F(255)), d), "Unsupported image format.")  # Integrate's
    # the pipeline goes on where it was
    assert pipe.process_frame(frames[2]) is True and pipe.frame_id == 3
    assert np.linalg.norm(np.asarray(pipe.cur_pose, np.float64) - run["pipe_pose"][2]) <= 1e-5
    # reset: a first frame with the bytes of a fresh pipeline's
    pipe.reset()
    assert pipe.frame_id == 0 and np.array_equal(pipe.cur_pose, np.eye(4, dtype=F)) and pipe.model_pyramid == []
    assert not pipe.volume.get_voxels()[1].any()
    assert pipe.process_frame(frames[0]) is True and pipe.frame_id == 1
    for a, b in zip(pipe.volume.get_voxels(), run["voxels0"][0]):
        assert ks.same(a, b)
    assert all(ks.same_cloud(a, b) for a, b in zip(pipe.model_pyramid, run["model0"][0]))
    # an unsupported tf_type is the reference's: a line per level, the pose as it was, the frame integrated
    pipe.option.tf_type = registration.TransformationEstimationType.PointToPoint
    weight = pipe.volume.get_voxels()[1].sum()
    capsys.readouterr()
    assert pipe.process_frame(frames[1]) is True and pipe.frame_id == 2
    assert capsys.readouterr().out.count("[KinfuPipeline::PoseEstimation] Unsupported transformation type.") == ks.LEVELS
    assert np.array_equal(pipe.cur_pose, np.eye(4, dtype=F)) and pipe.volume.get_voxels()[1].sum() > weight


def test_colored_icp_moves_the_pose_toward_the_truth():
    """tf_type = ColoredICP on float-intensity colour (a Gray32 volume), two frames; the scene in centimetres, as the
    project's other coloured tracker test (the reference's fp32 colour-gradient fit is ill-conditioned at metre scale)"""
    from cupoch_amd import kinfu, registration
    S = 100.0
    opt = ks.option(S, color_type=2, tf_type=registration.TransformationEstimationType.ColoredICP)
    pipe = kinfu.KinfuPipeline(ks.intrinsic(), opt)
    for k in (0, 2):
        assert pipe.process_frame(ks.rgbd(*ks.render(k, S, texture=True))) is True
    truth = ks.true_pose(2, S)[0]
    before, after = ks.pose_error(np.eye(4), truth, S), ks.pose_error(pipe.cur_pose, truth, S)
    print("colored ICP: pose error %.4f at the identity, %.4f after the frame" % (before, after))
    assert pipe.frame_id == 2 and pipe.model_pyramid[0].has_colors()
    assert after < before
