"""Inputs the KinfuPipeline tests share: a scene of three mutually non-parallel planes and a sphere (tsdf_exact.
render_scene) with pixels without depth, so that all six degrees of freedom of the camera are constrained; a camera
that moves by a known motion of about a voxel length per frame; and the frame loop composed by hand from the mirror's public pieces
(create_pyramid, bilateral_filter_pyramid_depth, point_cloud_pyramid, pose_estimation, integrate, raycast per level),
which is what the pipeline is compared with."""
import numpy as np

import tsdf_exact as tx

F = np.float32
W, H, FX, FY, CX, CY = 64, 48, 60.0, 60.0, 31.5, 23.5
LEVELS, RES = 3, 64
# Raycast enters the volume through the box [0, length]^3 of the camera's frame minus the origin (include/mi_icp.h):
# the scene lies in the volume's upper octant, seen from in front of it
LENGTH, TRUNC = 3.0, 0.12
PLANES = [((0.0, 0.0, 1.0), 1.0), ((0.0, 0.8, 0.6), 1.5), ((0.8, 0.0, 0.6), 1.5)]
SPHERE = ((0.6, 0.6, 0.75), 0.2)
EYE = (0.75, 0.75, -1.2)
# Pixels without depth: every 97th of a diagonal pattern.  Image::Downsample averages a zero depth into the coarse
# levels, as the reference does, and with render_scene's own pattern (every 11th pixel) hardly a coarse pixel stays
# clean: the tracker of the reference itself then leaves the scene (error 0.96 after a motion of 0.18, by hand and in
# the pipeline alike).  With these it follows the camera to within 0.03.
HOLES = 97
STEP_T = (0.03, -0.02, 0.025)        # per frame: about 0.044 = 0.94 voxel lengths (3 / 64) ...
STEP_R = 0.01                        # ... and 0.01 rad about the camera's y axis


def true_pose(k, S=1.0):
    """camera -> world pose of frame k RELATIVE TO FRAME 0 (what cur_pose tracks), and the frame's extrinsic"""
    a = STEP_R * k
    P = np.eye(4)
    P[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    P[:3, 3] = (np.asarray(EYE) + k * np.asarray(STEP_T)) * S
    P0 = np.eye(4)
    P0[:3, 3] = np.asarray(EYE) * S
    return (np.linalg.inv(P0) @ P).astype(F), np.linalg.inv(P).astype(F)


def render(k, S=1.0, texture=False):
    """(depth float32 [H, W], colour) of frame k at scale S; colour uint8 x 3 (render_scene's pattern), or with
    `texture` a smooth world-space intensity as float32 [H, W]"""
    _, E = true_pose(k, S)
    planes = [(n, off * S) for n, off in PLANES]
    d, c = tx.render_scene(W, H, FX, FY, CX, CY, E, planes, (tuple(S * v for v in SPHERE[0]), SPHERE[1] * S), holes=False)
    ys, xs = np.mgrid[0:H, 0:W]
    d[(xs * 7 + ys * 13) % HOLES == 0] = 0.0
    if not texture:
        return d, c
    cam = np.stack([(xs - CX) / FX * d, (ys - CY) / FY * d, d, np.ones_like(d)], -1).astype(np.float64)
    p = cam @ np.linalg.inv(E.astype(np.float64)).T / S
    v = 0.5 + 0.25 * np.sin(3.0 * p[..., 0]) + 0.25 * np.cos(2.0 * p[..., 1] + p[..., 2])
    return d, np.ascontiguousarray(v.astype(F))


def intrinsic():
    from cupoch_amd import camera
    return camera.PinholeCameraIntrinsic(W, H, FX, FY, CX, CY)


def option(S=1.0, color_type=1, tf_type=None, levels=LEVELS):
    """the frame's camera starts at the origin of the pipeline's world: the volume's origin puts the scene's octant
    in front of it"""
    from cupoch_amd import kinfu, registration
    T = registration.TransformationEstimationType
    return kinfu.KinfuOption(num_pyramid_levels=levels, depth_cutoff=3.0 * S, distance_threshold=0.15 * S,
                             icp_iterations=(10, 10, 10), tf_type=T.PointToPlane if tf_type is None else tf_type,
                             tsdf_length=LENGTH * S, tsdf_resolution=RES, sdf_trunc=TRUNC * S, tsdf_color_type=color_type,
                             tsdf_origin=tuple(-S * v for v in EYE))


def rgbd(d, c):
    from cupoch_amd import geometry
    return geometry.RGBDImage(c, d)


def inverse(T):
    """utility::InverseTransform in fp32: R^T and -(R^T t), the sums left to right"""
    T = np.asarray(T, F).reshape(4, 4)
    inv = np.eye(4, dtype=F)
    inv[:3, :3] = T[:3, :3].T
    for r in range(3):
        inv[r, 3] = -((inv[r, 0] * T[0, 3] + inv[r, 1] * T[1, 3]) + inv[r, 2] * T[2, 3])
    return inv


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def same(a, b):
    """bit-equal arrays of float32, NaN positions included"""
    a, b = np.ascontiguousarray(to_np(a), F), np.ascontiguousarray(to_np(b), F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def same_cloud(a, b):
    return same(a.points, b.points) and same(a.normals, b.normals) and same(a.colors, b.colors)


def measure(image, K, opt):
    """SurfaceMeasurement by hand -> (filtered pyramid, cloud pyramid)"""
    from cupoch_amd import geometry, kinfu
    pyramid = image.create_pyramid(opt.num_pyramid_levels)
    smooth = geometry.RGBDImage.bilateral_filter_pyramid_depth(pyramid, opt.diameter, opt.sigma_depth, opt.sigma_space)
    return smooth, kinfu.point_cloud_pyramid([s.depth for s in smooth], K, opt, [s.color for s in smooth])


class HandLoop:
    """kinfu.cpp:51-76 from the public pieces the project had before the pipeline"""

    def __init__(self, K, opt):
        from cupoch_amd import kinfu
        self.K, self.opt = K, opt
        self.volume = kinfu.create_volume(opt)
        self.pose = np.eye(4, dtype=F)
        self.model = []
        self.frames = 0

    def process(self, image):
        from cupoch_amd import kinfu
        smooth, clouds = measure(image, self.K, self.opt)
        E = inverse(self.pose)
        if self.frames > 0:
            E, _ = kinfu.pose_estimation(self.opt, E, self.model, clouds)
            self.pose = inverse(E)
        assert self.volume.integrate(smooth[0], self.K, E)
        self.model = [self.volume.raycast(self.K.create_pyramid_level(i), E, self.opt.sdf_trunc)
                      for i in range(self.opt.num_pyramid_levels)]
        self.frames += 1
        return clouds


def pose_error(T, truth, S=1.0):
    D = np.asarray(T, np.float64) - np.asarray(truth, np.float64)
    D[:3, 3] /= S
    return float(np.linalg.norm(D))
