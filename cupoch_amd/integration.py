"""cupoch.integration mirror (src/cupoch/integration/tsdfvolume.h, uniform_tsdfvolume.h; python surface
src/python/cupoch_pybind/integration/integration.cpp): TSDFVolumeColorType and UniformTSDFVolume.  The volume lives
on the GPU, owned by the process-wide engine of its device; every operation runs HIP kernels through the C ABI
(include/mi_icp.h has the numeric contract).  ScalableTSDFVolume is in cupoch_amd.integration_scalable (this module's
names are pinned by its surface test).  Not built: extract_triangle_mesh (no TriangleMesh type here),
extract_voxel_grid, integrate_with_depth_to_camera_distance_multiplier."""
import enum

import numpy as np

from . import geometry, utility
from ._lib import MiIcpError


class TSDFVolumeColorType(enum.IntEnum):
    NoColor = 0
    RGB8 = 1
    Gray32 = 2


def _cloud(p, n, c):
    out = geometry.PointCloud()
    out._points = utility.Vector3fVector(p)
    if n is not None:
        out._normals = utility.Vector3fVector(n)
    if c is not None:
        out._colors = utility.Vector3fVector(c)
    return out


class TSDFVolume:
    """tsdfvolume.h:44-74: the base class's fields, and what the two volumes do alike.  A subclass names the
    reference's class (_LABEL) and the prefix of its engine functions (_API), and keeps its engine and handle in _eng
    and _vol."""
    _LABEL = _API = _vol = None

    def __init__(self, voxel_length, sdf_trunc, color_type):
        self.voxel_length = float(np.float32(voxel_length))
        self.sdf_trunc = float(np.float32(sdf_trunc))
        self.color_type = TSDFVolumeColorType(color_type)

    def _call(self, name, *args):
        return getattr(self._eng, self._API + name)(self._vol, *args)

    def __del__(self):
        try:
            self._call("_destroy")
        except Exception:
            pass
        self._vol = None

    def reset(self):
        self._call("_reset")

    def integrate(self, image, intrinsic, extrinsic):
        """<class>::Integrate(RGBDImage, PinholeCameraIntrinsic, extrinsic).  Returns True; a format the reference turns
        away ([<class>::Integrate] Unsupported image format.) is reported, the volume is left as it was and False
        comes back."""
        bad = "[%s::Integrate] Unsupported image format." % self._LABEL
        color = None if self.color_type == TSDFVolumeColorType.NoColor else image.color
        try:
            if color is None and self.color_type != TSDFVolumeColorType.NoColor:
                raise MiIcpError(bad)
            self._call("_integrate", image.depth, color, intrinsic.width, intrinsic.height, intrinsic.as4(), extrinsic)
        except MiIcpError as e:
            if "Unsupported image format" not in str(e):
                raise
            print("[cupoch_amd] Error: " + bad)
            return False
        return True

    def extract_point_cloud(self):
        p, n, c = self._call("_extract_point_cloud", self.color_type != TSDFVolumeColorType.NoColor)
        return _cloud(p, n, c)

    def extract_voxel_point_cloud(self):
        p, c = self._call("_extract_voxel_point_cloud")
        return _cloud(p, None, c)


class UniformTSDFVolume(TSDFVolume):
    _LABEL, _API = "UniformTSDFVolume", "tsdf"

    def __init__(self, length, resolution, sdf_trunc, color_type, origin=(0.0, 0.0, 0.0), device=None):
        color_type = TSDFVolumeColorType(color_type)
        resolution = int(resolution)
        super().__init__(np.float32(length) / np.float32(resolution), sdf_trunc, color_type)
        self.length = float(np.float32(length))
        self.resolution = resolution
        self.voxel_num = resolution * resolution * resolution
        self.origin = np.asarray(origin, np.float32).reshape(3).copy()
        self._eng = geometry.get_engine(device)
        self._vol = self._eng.tsdf_create(self.length, resolution, self.sdf_trunc, int(color_type), self.origin)

    def raycast(self, intrinsic, extrinsic, sdf_trunc, project_valid_depth_only=True):
        p, n, c = self._eng.tsdf_raycast(self._vol, intrinsic.width, intrinsic.height, intrinsic.as4(), extrinsic,
                                         sdf_trunc, project_valid_depth_only)
        return _cloud(p, n, c)

    def raycast_levels(self, intrinsic, extrinsic, sdf_trunc, levels, project_valid_depth_only=True):
        """[raycast(intrinsic.create_pyramid_level(i), extrinsic, sdf_trunc, project_valid_depth_only) for i in
        range(levels)], the same bytes, in one pass over the volume (mi_icp_tsdf_raycast_levels)"""
        return [_cloud(p, n, c) for p, n, c in self._eng.tsdf_raycast_levels(
            self._vol, levels, intrinsic.width, intrinsic.height, intrinsic.as4(), extrinsic, sdf_trunc,
            project_valid_depth_only)]

    def get_voxels(self):
        """(tsdf[n], weight[n], color[n, 3]) as numpy arrays, n = resolution^3 indexed x*res*res + y*res + z; a
        NoColor volume reports the colour every voxel starts with, (1, 1, 1)"""
        t, w, c = self._eng.tsdf_get_voxels(self._vol, self.voxel_num, self.color_type != TSDFVolumeColorType.NoColor)
        if c is None:
            c = np.ones((self.voxel_num, 3), np.float32)
        return t, w, c
