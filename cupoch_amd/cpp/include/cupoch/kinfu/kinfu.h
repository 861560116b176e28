// cupoch/kinfu/kinfu.h -- kinfu::KinfuOption and kinfu::KinfuPipeline (reference: kinfu/kinfu.h:36-121,
// kinfu.cpp:29-143): the KinectFusion frame loop over integration::UniformTSDFVolume
// (cupoch/integration/uniform_tsdfvolume.h), the image pyramid and bilateral depth filter of
// cupoch/geometry/image.h and the registrations.  The point-cloud pyramid of SurfaceMeasurement and the
// coarse-to-fine PoseEstimation are also free functions taking the option block.  DESIGN.md 4.14 has the
// data flow of a frame.  Not declared: ExtractTriangleMesh (no TriangleMesh type here).
#pragma once
#include <memory>
#include <tuple>
#include <vector>

#include "cupoch/camera/pinhole_camera_intrinsic.h"
#include "cupoch/geometry/image.h"
#include "cupoch/geometry/pointcloud.h"
#include "cupoch/integration/uniform_tsdfvolume.h"
#include "cupoch/registration/transformation_estimation.h"

namespace cupoch {
namespace kinfu {

typedef std::vector<std::shared_ptr<geometry::PointCloud>> PointCloudPyramid;

/// kinfu.h:36-80 with the reference's defaults.  The constructor takes the five fields the registrations read;
/// the others are set as members (the reference's Python surface has a default constructor and fields only).
class KinfuOption {
public:
    KinfuOption(int num_pyramid_levels = 4,
                float depth_cutoff = 3.0f,
                float distance_threshold = 0.5f,
                const std::vector<int>& icp_iterations = {20, 20, 20, 20},
                registration::TransformationEstimationType tf_type =
                        registration::TransformationEstimationType::PointToPlane)
        : num_pyramid_levels_(num_pyramid_levels),
          depth_cutoff_(depth_cutoff),
          distance_threshold_(distance_threshold),
          icp_iterations_(icp_iterations),
          tf_type_(tf_type) {}
    int num_pyramid_levels_;
    int diameter_ = 1;
    float sigma_depth_ = 1.0f;
    float sigma_space_ = 10.0f;
    float depth_cutoff_;
    float tsdf_length_ = 8.0f;
    int tsdf_resolution_ = 512;
    float sdf_trunc_ = 0.05f;
    integration::TSDFVolumeColorType tsdf_color_type_ = integration::TSDFVolumeColorType::RGB8;
    Eigen::Vector3f tsdf_origin_ = Eigen::Vector3f::Zero();
    float distance_threshold_;
    std::vector<int> icp_iterations_;
    registration::TransformationEstimationType tf_type_;
};

/// kinfu.cpp:95-100: level i of an (already filtered) RGB-D pyramid ->
/// CreateFromRGBDImage(level, intrinsic.CreatePyramidLevel(i), I, true, depth_cutoff, true)
PointCloudPyramid CreatePointCloudPyramid(const std::vector<geometry::RGBDImage>& image_pyramid,
                                          const camera::PinholeCameraIntrinsic& intrinsic,
                                          const KinfuOption& option);
PointCloudPyramid CreatePointCloudPyramid(const geometry::RGBDImagePyramid& image_pyramid,
                                          const camera::PinholeCameraIntrinsic& intrinsic,
                                          const KinfuOption& option);

/// KinfuPipeline::PoseEstimation (kinfu.cpp:105-143)
std::tuple<Eigen::Matrix4f, bool> PoseEstimation(const KinfuOption& option,
                                                 const Eigen::Matrix4f& extrinsic,
                                                 const PointCloudPyramid& frame_data,
                                                 const PointCloudPyramid& target_data);

/// kinfu.h:82-111.  Not copyable (UniformTSDFVolume is not).
class KinfuPipeline {
public:
    /// at most this many pyramid levels (MI_ICP_TSDF_MAX_LEVELS: one raycast serves them all)
    static constexpr int kMaxPyramidLevels = 16;

    KinfuPipeline(const camera::PinholeCameraIntrinsic& intrinsic, const KinfuOption& option = KinfuOption());
    ~KinfuPipeline();

    /// identity pose, a reset volume, no model pyramid, frame_id_ = 0
    void Reset();
    /// kinfu.cpp:51-76.  Where the reference reads out of bounds or goes on with garbage the call is refused:
    /// "[KinfuPipeline::ProcessFrame] ..." is logged, false comes back, and pose, volume, model pyramid and
    /// frame_id_ are as they were -- colour or depth without data, num_pyramid_levels_ outside
    /// [1, kMaxPyramidLevels], fewer icp_iterations_ than levels, a frame whose size is not the intrinsic's, an
    /// image format the pyramid or Integrate turns away.
    bool ProcessFrame(const geometry::RGBDImage& image);
    std::shared_ptr<geometry::PointCloud> ExtractPointCloud();

public:
    camera::PinholeCameraIntrinsic intrinsic_;
    Eigen::Matrix4f cur_pose_ = Eigen::Matrix4f::Identity();
    int frame_id_ = 0;
    integration::UniformTSDFVolume volume_;
    PointCloudPyramid model_pyramid_;
    KinfuOption option_;
};

}  // namespace kinfu
}  // namespace cupoch
