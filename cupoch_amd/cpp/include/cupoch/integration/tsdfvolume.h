// cupoch/integration/tsdfvolume.h -- integration::TSDFVolumeColorType and the TSDFVolume interface
// (reference: integration/tsdfvolume.h:31-74).  ExtractTriangleMesh is not part of it here: there
// is no geometry::TriangleMesh type in this surface.
#pragma once
#include <memory>

#include "cupoch/camera/pinhole_camera_intrinsic.h"
#include "cupoch/geometry/image.h"
#include "cupoch/geometry/pointcloud.h"

namespace cupoch {
namespace integration {

enum class TSDFVolumeColorType {
    NoColor = 0,
    RGB8 = 1,
    Gray32 = 2,
};

class TSDFVolume {
public:
    TSDFVolume(float voxel_length, float sdf_trunc, TSDFVolumeColorType color_type)
        : voxel_length_(voxel_length), sdf_trunc_(sdf_trunc), color_type_(color_type) {}
    virtual ~TSDFVolume() {}

public:
    virtual void Reset() = 0;
    virtual void Integrate(const geometry::RGBDImage& image, const camera::PinholeCameraIntrinsic& intrinsic,
                           const Eigen::Matrix4f& extrinsic) = 0;
    virtual std::shared_ptr<geometry::PointCloud> ExtractPointCloud() = 0;

public:
    float voxel_length_;
    float sdf_trunc_;
    TSDFVolumeColorType color_type_;
};

}  // namespace integration
}  // namespace cupoch
