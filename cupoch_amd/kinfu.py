"""The ICP and volume sides of cupoch.kinfu.KinfuPipeline (src/cupoch/kinfu/kinfu.h:36-121, kinfu.cpp:51-143): the
depth-frame -> point-cloud pyramid of SurfaceMeasurement, the coarse-to-fine PoseEstimation that calls
RegistrationICP / RegistrationColoredICP once per pyramid level, and the two volume steps of ProcessFrame
(Integrate, then one Raycast per pyramid level).  The image pyramid and the bilateral depth filter that ProcessFrame
needs in front of them exist now (geometry.RGBDImage.create_pyramid / bilateral_filter_pyramid_depth);
ProcessFrame as a whole is still not composed from these pieces."""
import numpy as np

from . import geometry, registration
from .integration import TSDFVolumeColorType, UniformTSDFVolume
from .registration import TransformationEstimationType


class KinfuOption:
    """kinfu.h:36-82, the fields PoseEstimation / SurfaceMeasurement and the volume read (diameter, sigma_depth and
    sigma_space belong to the bilateral filter, geometry.RGBDImage.bilateral_filter_pyramid_depth, which ProcessFrame would
    call; it is not composed here)."""

    def __init__(self, num_pyramid_levels=4, depth_cutoff=3.0, distance_threshold=0.5,
                 icp_iterations=(20, 20, 20, 20), tf_type=TransformationEstimationType.PointToPlane,
                 tsdf_length=8.0, tsdf_resolution=512, sdf_trunc=0.05, tsdf_color_type=TSDFVolumeColorType.RGB8,
                 tsdf_origin=(0.0, 0.0, 0.0)):
        self.num_pyramid_levels = int(num_pyramid_levels)
        self.depth_cutoff = float(depth_cutoff)
        self.distance_threshold = float(distance_threshold)
        self.icp_iterations = list(icp_iterations)
        self.tf_type = tf_type
        self.tsdf_length = float(tsdf_length)
        self.tsdf_resolution = int(tsdf_resolution)
        self.sdf_trunc = float(sdf_trunc)
        self.tsdf_color_type = TSDFVolumeColorType(tsdf_color_type)
        self.tsdf_origin = np.asarray(tsdf_origin, np.float32).reshape(3)


def create_volume(option, device=None):
    """KinfuPipeline's volume_ (kinfu.cpp:32-36)"""
    return UniformTSDFVolume(option.tsdf_length, option.tsdf_resolution, option.sdf_trunc, option.tsdf_color_type,
                             option.tsdf_origin, device)


def integrate_and_raycast(volume, option, image, intrinsic, extrinsic):
    """ProcessFrame's volume steps (kinfu.cpp:69-73): volume.Integrate(image, intrinsic, extrinsic), then
    volume.Raycast(intrinsic.CreatePyramidLevel(i), extrinsic, sdf_trunc) for every level -- the model pyramid that
    pose_estimation takes as target_data for the next frame.  None when the frame's format is turned away."""
    if not volume.integrate(image, intrinsic, extrinsic):
        return None
    return [volume.raycast(intrinsic.create_pyramid_level(i), extrinsic, option.sdf_trunc)
            for i in range(option.num_pyramid_levels)]


def point_cloud_pyramid(depth_pyramid, intrinsic, option, color_pyramid=None):
    """SurfaceMeasurement's last loop (kinfu.cpp:95-100): level i of the (already filtered)
    depth pyramid -> CreateFromRGBDImage(level image, intrinsic.CreatePyramidLevel(i), Identity,
    true, depth_cutoff, true)."""
    out = []
    for i in range(option.num_pyramid_levels):
        col = None if color_pyramid is None else color_pyramid[i]
        out.append(geometry.PointCloud.create_from_rgbd_image(
            geometry.RGBDImage(col, depth_pyramid[i]), intrinsic.create_pyramid_level(i), np.eye(4, dtype=np.float32),
            True, option.depth_cutoff, True))
    return out


def pose_estimation(option, extrinsic, frame_data, target_data):
    """KinfuPipeline::PoseEstimation (kinfu.cpp:105-143).  Returns (transformation, success)."""
    cur = np.asarray(extrinsic, np.float32).reshape(4, 4).copy()
    for level in range(option.num_pyramid_levels - 1, -1, -1):
        criteria = registration.ICPConvergenceCriteria()
        criteria.max_iteration = option.icp_iterations[level]
        if option.tf_type == TransformationEstimationType.PointToPlane:
            res = registration.registration_icp(
                frame_data[level], target_data[level], option.distance_threshold, cur,
                registration.TransformationEstimationPointToPlane(100000), criteria)
            cur = np.asarray(res.transformation, np.float32)
        elif option.tf_type == TransformationEstimationType.ColoredICP:
            res = registration.registration_colored_icp(
                frame_data[level], target_data[level], option.distance_threshold, cur, criteria,
                0.968, 100000)
            cur = np.asarray(res.transformation, np.float32)
        else:
            print("[cupoch_amd] Error: [KinfuPipeline::PoseEstimation] Unsupported transformation type.")
    return cur, True
