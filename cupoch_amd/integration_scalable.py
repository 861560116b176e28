"""cupoch.integration.ScalableTSDFVolume (src/cupoch/integration/scalable_tsdfvolume.h; python surface
src/python/cupoch_pybind/integration/integration.cpp:153-195), beside cupoch_amd.integration, whose TSDFVolume and
TSDFVolumeColorType it uses.  The volume lives on the GPU, owned by the process-wide engine of its device; every
operation runs HIP kernels through the C ABI (include/mi_icp.h has the numeric contract).  Not built:
extract_triangle_mesh (the reference's own is a stub that logs an error), a raycast (the reference has none),
integrate_with_depth_to_camera_distance_multiplier."""
import numpy as np

from . import geometry
from .integration import TSDFVolume, TSDFVolumeColorType


class ScalableTSDFVolume(TSDFVolume):
    """scalable_tsdfvolume.h: a sparse volume of 16^3-voxel units opened around the observed surface.  map_size is the
    initial number of unit slots: the volume grows by doubling where the reference drops units."""
    _LABEL, _API = "ScalableTSDFVolume", "stsdf"

    def __init__(self, voxel_length, sdf_trunc, color_type, depth_sampling_stride=4, map_size=1000, device=None):
        color_type = TSDFVolumeColorType(color_type)
        super().__init__(voxel_length, sdf_trunc, color_type)
        self.resolution = 16
        self.volume_unit_length = float(np.float32(voxel_length) * np.float32(16.0))
        self.volume_unit_voxel_num = 4096
        self.depth_sampling_stride = int(depth_sampling_stride)
        self._eng = geometry.get_engine(device)
        self._vol = self._eng.stsdf_create(self.voxel_length, self.sdf_trunc, int(color_type), self.depth_sampling_stride,
                                           int(map_size))

    def num_volume_units(self):
        """(open units, unit slots allocated)"""
        return self._eng.stsdf_num_units(self._vol)

    def get_volume_units(self):
        """(keys[m, 3] int32 in ascending (x, y, z) order, tsdf[m, 4096], weight[m, 4096], color[m, 4096, 3]) as numpy
        arrays, a voxel at x*256 + y*16 + z of its unit; a NoColor volume reports the colour every voxel starts with"""
        k, t, w, c = self._eng.stsdf_get_units(self._vol, self.color_type != TSDFVolumeColorType.NoColor)
        if c is None:
            c = np.ones((len(k), 4096, 3), np.float32)
        return k, t, w, c
