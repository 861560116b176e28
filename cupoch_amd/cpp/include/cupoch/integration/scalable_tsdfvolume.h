// cupoch/integration/scalable_tsdfvolume.h -- integration::ScalableTSDFVolume (reference:
// integration/scalable_tsdfvolume.h:51-103) over mi_icp_stsdf_* (include/mi_icp.h has the numeric
// contract): units of 16^3 voxels opened around the observed surface, in the engine's context.  The
// units are read back with GetVolumeUnits() instead of a public hash map, in ascending key order.
// map_size is the initial number of unit slots: the volume grows by doubling where the reference's map
// drops units.  Not built: ExtractTriangleMesh (the reference's own only logs an error),
// IntegrateWithDepthToCameraDistanceMultiplier as a public entry.
#pragma once
#include <vector>

#include "cupoch/integration/uniform_tsdfvolume.h"

struct mi_icp_stsdf;

namespace cupoch {
namespace integration {

class ScalableTSDFVolume : public TSDFVolume {
public:
    /// One open unit: its key (the unit spans key * volume_unit_length_ to (key + 1) * volume_unit_length_)
    /// and its 4096 voxels, indexed x*256 + y*16 + z (a NoColor volume reports colour (1, 1, 1)).
    struct VolumeUnit {
        Eigen::Vector3i index_;
        std::vector<geometry::TSDFVoxel> voxels_;
    };

public:
    ScalableTSDFVolume(float voxel_length, float sdf_trunc, TSDFVolumeColorType color_type,
                       int depth_sampling_stride = 4, int map_size = 1000);
    ~ScalableTSDFVolume() override;
    ScalableTSDFVolume(const ScalableTSDFVolume&) = delete;
    ScalableTSDFVolume& operator=(const ScalableTSDFVolume&) = delete;

public:
    void Reset() override;
    /// An image format the reference turns away is logged
    /// ("[ScalableTSDFVolume::Integrate] Unsupported image format.") and leaves the volume as it was.
    void Integrate(const geometry::RGBDImage& image, const camera::PinholeCameraIntrinsic& intrinsic,
                   const Eigen::Matrix4f& extrinsic) override;
    std::shared_ptr<geometry::PointCloud> ExtractPointCloud() override;
    /// Debug function to extract the voxel data into a point cloud.
    std::shared_ptr<geometry::PointCloud> ExtractVoxelPointCloud();
    /// the open units in ascending (x, y, z) key order
    std::vector<VolumeUnit> GetVolumeUnits() const;
    size_t NumVolumeUnits() const;

public:
    float volume_unit_length_;
    int resolution_;
    int volume_unit_voxel_num_;
    int depth_sampling_stride_;

private:
    mi_icp_stsdf* volume_ = nullptr;
};

}  // namespace integration
}  // namespace cupoch
