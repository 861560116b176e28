// cupoch/integration/uniform_tsdfvolume.h -- integration::UniformTSDFVolume (reference:
// integration/uniform_tsdfvolume.h:30-89) over mi_icp_tsdf_* (include/mi_icp.h has the numeric
// contract).  The voxels live in the engine's context as planes; GetVoxels() reads them back in the
// reference's TSDFVoxel form instead of a public voxels_ vector.
// Not built: ExtractTriangleMesh (no TriangleMesh type here), ExtractVoxelGrid,
// IntegrateWithDepthToCameraDistanceMultiplier as a public entry.  ScalableTSDFVolume is in
// cupoch/integration/scalable_tsdfvolume.h.
#pragma once
#include <vector>

#include "cupoch/integration/tsdfvolume.h"

struct mi_icp_tsdf;

namespace cupoch {
namespace geometry {

class TSDFVoxel {
public:
    float tsdf_ = 0;
    float weight_ = 0;
    Eigen::Vector3f color_ = Eigen::Vector3f(1.0f, 1.0f, 1.0f);
};

}  // namespace geometry

namespace integration {

class UniformTSDFVolume : public TSDFVolume {
public:
    UniformTSDFVolume(float length, int resolution, float sdf_trunc, TSDFVolumeColorType color_type,
                      const Eigen::Vector3f& origin = Eigen::Vector3f::Zero());
    ~UniformTSDFVolume() override;
    UniformTSDFVolume(const UniformTSDFVolume&) = delete;  // (the reference copies the voxels; not provided)
    UniformTSDFVolume& operator=(const UniformTSDFVolume&) = delete;

public:
    void Reset() override;
    /// An image format the reference turns away is logged
    /// ("[UniformTSDFVolume::Integrate] Unsupported image format.") and leaves the volume as it was.
    void Integrate(const geometry::RGBDImage& image, const camera::PinholeCameraIntrinsic& intrinsic,
                   const Eigen::Matrix4f& extrinsic) override;
    /// Integrate; false (after the same log line) when the format was turned away
    bool TryIntegrate(const geometry::RGBDImage& image, const camera::PinholeCameraIntrinsic& intrinsic,
                      const Eigen::Matrix4f& extrinsic);
    std::shared_ptr<geometry::PointCloud> ExtractPointCloud() override;
    std::shared_ptr<geometry::PointCloud> ExtractVoxelPointCloud() const;
    std::shared_ptr<geometry::PointCloud> Raycast(const camera::PinholeCameraIntrinsic& intrinsic,
                                                  const Eigen::Matrix4f& extrinsic, float sdf_trunc,
                                                  bool project_valid_depth_only = true) const;
    /// Raycast(intrinsic.CreatePyramidLevel(i), extrinsic, sdf_trunc, project_valid_depth_only) for i = 0 .. levels-1,
    /// the same values, in one pass over the volume (mi_icp_tsdf_raycast_levels); 1 <= levels <= 16
    std::vector<std::shared_ptr<geometry::PointCloud>> RaycastLevels(const camera::PinholeCameraIntrinsic& intrinsic,
                                                                     const Eigen::Matrix4f& extrinsic, float sdf_trunc,
                                                                     int levels, bool project_valid_depth_only = true) const;
    /// voxel_num_ voxels, indexed x*res*res + y*res + z (a NoColor volume reports colour (1, 1, 1))
    std::vector<geometry::TSDFVoxel> GetVoxels() const;

public:
    Eigen::Vector3f origin_;
    float length_;
    int resolution_;
    int voxel_num_;

private:
    mi_icp_tsdf* volume_ = nullptr;
};

}  // namespace integration
}  // namespace cupoch
