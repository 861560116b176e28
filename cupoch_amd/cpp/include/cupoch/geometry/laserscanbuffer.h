// cupoch/geometry/laserscanbuffer.h -- geometry::LaserScanBuffer (reference: geometry/laserscanbuffer.h): a ring of
// scans from a planar laser range-finder, each with the pose (origin) it was taken from; the two filters, the two
// "virtual lidar" factories and, in pointcloud.h, PointCloud::CreateFromLaserScanBuffer.  The conversions and filters run
// on the GPU through the mi_icp_laserscan_* family; the contract is in include/mi_icp.h ("laserscan").
//
// THE RING.  ranges_ (and intensities_, when the buffer has them) are device storage of num_max_scans_ x num_steps_
// readings, made with the first scan; origins_ is HOST memory, one matrix per slot (the engine takes origins from the
// host).  The newest scan goes to slot bottom_ % num_max_scans_; a full ring overwrites its oldest scan and advances
// top_; the live scans are slots top_ .. bottom_ - 1 (mod num_max_scans_), oldest first.  A buffer has intensities when
// the first scan added to it while empty carried them.  GetRanges / GetIntensities return the live scans oldest first
// (the reference's GetIntensities computes a negative length); Merge appends the other buffer's live scans oldest
// first; RangeFilter and ScanShadowsFilter return a buffer that keeps origins, intensities, top_ and bottom_ (the
// reference's RangeFilter drops origins and intensities); ScanShadowsFilter compares inside the reading's own scan (the
// reference compares inside scan 0).  The factories return max(DEFAULT_NUM_MAX_SCANS, divisions) slots, of which
// `divisions` are live.
#pragma once
#include <cmath>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

#include "cupoch/camera/pinhole_camera_intrinsic.h"
#include "cupoch/geometry/image.h"
#include "cupoch/geometry/pointcloud.h"

namespace cupoch {
namespace utility {
template <typename T>
using pinned_host_vector = std::vector<T>;
}
namespace geometry {

static const unsigned int DEFAULT_NUM_MAX_SCANS = 50;

class LaserScanBuffer : public GeometryBase3D {
public:
    LaserScanBuffer(int num_steps, int num_max_scans = DEFAULT_NUM_MAX_SCANS, float min_angle = -M_PI, float max_angle = M_PI);
    ~LaserScanBuffer() override;
    LaserScanBuffer(const LaserScanBuffer& other);

    /// the live scans, oldest first
    thrust::host_vector<float> GetRanges() const;
    thrust::host_vector<float> GetIntensities() const;

    LaserScanBuffer& Clear() override;
    bool IsEmpty() const override;
    /// the four bounds getters log "not supported" and return zeros, as the reference's do
    Eigen::Vector3f GetMinBound() const override;
    Eigen::Vector3f GetMaxBound() const override;
    Eigen::Vector3f GetCenter() const override;
    AxisAlignedBoundingBox<3> GetAxisAlignedBoundingBox() const override;
    /// O <- O * T for every origin
    LaserScanBuffer& Transform(const Eigen::Matrix4f& transformation) override;
    LaserScanBuffer& Translate(const Eigen::Vector3f& translation, bool relative = true) override;
    /// multiplies the ranges
    LaserScanBuffer& Scale(const float scale, bool center = true) override;
    LaserScanBuffer& Rotate(const Eigen::Matrix3f& R, bool center = true) override;

    bool HasIntensities() const { return !intensities_.empty(); }
    float GetAngleIncrement() const { return (max_angle_ - min_angle_) / (float)(num_steps_ - 1); }
    bool IsFull() const { return GetNumScans() == num_max_scans_; }
    int GetNumScans() const { return bottom_ - top_; }

    LaserScanBuffer& AddRanges(const utility::device_vector<float>& ranges,
                               const Eigen::Matrix4f& transformation = Eigen::Matrix4f::Identity(),
                               const utility::device_vector<float>& intensities = utility::device_vector<float>());
    LaserScanBuffer& AddRanges(const thrust::host_vector<float>& ranges,
                               const Eigen::Matrix4f& transformation = Eigen::Matrix4f::Identity(),
                               const thrust::host_vector<float>& intensities = thrust::host_vector<float>());
    /// num_steps_ readings in host memory
    LaserScanBuffer& AddRanges(const float* ranges, const Eigen::Matrix4f& transformation = Eigen::Matrix4f::Identity(),
                               const float* intensities = nullptr);

    LaserScanBuffer& Merge(const LaserScanBuffer& other);

    std::shared_ptr<LaserScanBuffer> PopOneScan();
    std::pair<std::unique_ptr<utility::pinned_host_vector<float>>, std::unique_ptr<utility::pinned_host_vector<float>>> PopHostOneScan();

    std::shared_ptr<LaserScanBuffer> RangeFilter(float min_range, float max_range) const;
    std::shared_ptr<LaserScanBuffer> ScanShadowsFilter(float min_angle, float max_angle, int window, int neighbors = 0,
                                                       bool remove_shadow_start_point = false) const;

    static std::shared_ptr<LaserScanBuffer> CreateFromPointCloud(const geometry::PointCloud& pcd, float angle_increment,
                                                                 float min_height, float max_height,
                                                                 unsigned int num_vertical_divisions = 1, float min_range = 0.0,
                                                                 float max_range = std::numeric_limits<float>::infinity(),
                                                                 float min_angle = -M_PI, float max_angle = M_PI);
    static std::shared_ptr<LaserScanBuffer> CreateFromDepthImage(const geometry::Image& depth,
                                                                 const camera::PinholeCameraIntrinsic& intrinsic,
                                                                 float angle_increment, float min_y, float max_y,
                                                                 unsigned int num_vertical_divisions = 1, float min_range = 0.0,
                                                                 float max_range = std::numeric_limits<float>::infinity(),
                                                                 float min_angle = -M_PI, float max_angle = M_PI,
                                                                 float depth_scale = 1000.0, float depth_trunc = 1000.0,
                                                                 int stride = 1);

public:
    utility::device_vector<float> ranges_;       // [num_max_scans_][num_steps_] once a scan has been added
    utility::device_vector<float> intensities_;  // the same shape, or empty
    int top_ = 0;     //!< index of the oldest scan
    int bottom_ = 0;  //!< index of the newest scan
    const int num_steps_;      //!< number of steps in a scan
    const int num_max_scans_;  //!< maximum number of scans
    float min_angle_;
    float max_angle_;
    std::vector<Eigen::Matrix4f> origins_;       // [num_max_scans_], host memory
};

}  // namespace geometry
}  // namespace cupoch
