// cupoch/geometry/pointcloud.h -- geometry::PointCloud as the ICP path sees it
// (reference: geometry/pointcloud.h:43-263, geometry/geometry_base.h,
// geometry/geometry.h).  Same public members and layouts; the operations run
// HIP kernels through libmi_icp.so's C ABI (include/mi_icp.h).
#pragma once
#include <cmath>
#include <memory>
#include <tuple>

#include "cupoch/camera/pinhole_camera_intrinsic.h"
#include "cupoch/geometry/image.h"
#include "cupoch/knn/kdtree_search_param.h"
#include "cupoch/utility/device_vector.h"
#include "cupoch/utility/eigen.h"

namespace cupoch {
namespace geometry {

class Geometry {
public:
    enum class GeometryType { Unspecified = 0, PointCloud = 1, VoxelGrid = 2, OccupancyGrid = 3, DistanceTransform = 4, LineSet = 5, Graph = 6, AxisAlignedBoundingBox = 13, LaserScanBuffer = 14 };  // geometry.h:37-68
    virtual ~Geometry() {}
    GeometryType GetGeometryType() const { return type_; }
    int Dimension() const { return dimension_; }
    virtual Geometry& Clear() = 0;
    virtual bool IsEmpty() const = 0;

protected:
    Geometry(GeometryType type, int dimension) : type_(type), dimension_(dimension) {}

private:
    GeometryType type_;
    int dimension_;
};

class AxisAlignedBoundingBox3;
class OccupancyGrid;
class LaserScanBuffer;

/// geometry/geometry_base.h:33-90 with VectorT = Vector3f, MatrixT = Matrix3f, TransformT = Matrix4f
class GeometryBase3D : public Geometry {
protected:
    GeometryBase3D(GeometryType type) : Geometry(type, 3) {}

public:
    GeometryBase3D& Clear() override = 0;
    bool IsEmpty() const override = 0;
    virtual Eigen::Vector3f GetMinBound() const = 0;
    virtual Eigen::Vector3f GetMaxBound() const = 0;
    virtual Eigen::Vector3f GetCenter() const = 0;
    virtual AxisAlignedBoundingBox3 GetAxisAlignedBoundingBox() const = 0;
    virtual GeometryBase3D& Transform(const Eigen::Matrix4f& transformation) = 0;
    virtual GeometryBase3D& Translate(const Eigen::Vector3f& translation, bool relative = true) = 0;
    virtual GeometryBase3D& Scale(const float scale, bool center = true) = 0;
    virtual GeometryBase3D& Rotate(const Eigen::Matrix3f& R, bool center = true) = 0;
};

/// geometry::AxisAlignedBoundingBox<3> (geometry/boundingvolume.h:121-230): the value
/// PointCloud::GetAxisAlignedBoundingBox hands out -- bounds, centre, extent, volume and the
/// GeometryBase3D moves of a box (geometry/boundingvolume.cu; Rotate is not defined for an
/// axis-aligned box and logs an error there as here).
class AxisAlignedBoundingBox3 : public GeometryBase3D {
public:
    AxisAlignedBoundingBox3()
        : GeometryBase3D(GeometryType::AxisAlignedBoundingBox),
          min_bound_(Eigen::Vector3f::Zero()), max_bound_(Eigen::Vector3f::Zero()), color_(Eigen::Vector3f::Zero()) {}
    AxisAlignedBoundingBox3(const Eigen::Vector3f& min_bound, const Eigen::Vector3f& max_bound)
        : GeometryBase3D(GeometryType::AxisAlignedBoundingBox),
          min_bound_(min_bound), max_bound_(max_bound), color_(Eigen::Vector3f::Zero()) {}
    AxisAlignedBoundingBox3& Clear() override {
        min_bound_ = max_bound_ = Eigen::Vector3f::Zero();
        return *this;
    }
    bool IsEmpty() const override { return Volume() <= 0; }
    Eigen::Vector3f GetMinBound() const override { return min_bound_; }
    Eigen::Vector3f GetMaxBound() const override { return max_bound_; }
    Eigen::Vector3f GetCenter() const override { return (min_bound_ + max_bound_) * 0.5f; }
    AxisAlignedBoundingBox3 GetAxisAlignedBoundingBox() const override;
    AxisAlignedBoundingBox3& Transform(const Eigen::Matrix4f& transformation) override;
    AxisAlignedBoundingBox3& Translate(const Eigen::Vector3f& translation, bool relative = true) override;
    AxisAlignedBoundingBox3& Scale(const float scale, bool center = true) override;
    AxisAlignedBoundingBox3& Rotate(const Eigen::Matrix3f& R, bool center = true) override;
    Eigen::Vector3f GetExtent() const { return max_bound_ - min_bound_; }
    Eigen::Vector3f GetHalfExtent() const { return GetExtent() * 0.5f; }
    float GetMaxExtent() const {
        const Eigen::Vector3f e = GetExtent();
        return std::fmax(e[0], std::fmax(e[1], e[2]));
    }
    float Volume() const {
        const Eigen::Vector3f e = GetExtent();
        return e[0] * e[1] * e[2];
    }

public:
    Eigen::Vector3f min_bound_, max_bound_, color_;
};
template <int Dim>
struct AxisAlignedBoundingBoxOf;
template <>
struct AxisAlignedBoundingBoxOf<3> {
    typedef AxisAlignedBoundingBox3 type;
};
/// the reference spells the 3-D box AxisAlignedBoundingBox<3>
template <int Dim>
using AxisAlignedBoundingBox = typename AxisAlignedBoundingBoxOf<Dim>::type;

class PointCloud : public GeometryBase3D {
public:
    PointCloud() : GeometryBase3D(GeometryType::PointCloud) {}
    PointCloud(const thrust::host_vector<Eigen::Vector3f>& points)
        : GeometryBase3D(GeometryType::PointCloud), points_(points) {}
    PointCloud(const PointCloud& other) = default;
    PointCloud& operator=(const PointCloud& other) = default;
    ~PointCloud() override {}

    void SetPoints(const thrust::host_vector<Eigen::Vector3f>& points) { points_ = points; }
    thrust::host_vector<Eigen::Vector3f> GetPoints() const { return points_.to_host(); }
    void SetNormals(const thrust::host_vector<Eigen::Vector3f>& normals) { normals_ = normals; }
    thrust::host_vector<Eigen::Vector3f> GetNormals() const { return normals_.to_host(); }
    void SetColors(const thrust::host_vector<Eigen::Vector3f>& colors) { colors_ = colors; }
    thrust::host_vector<Eigen::Vector3f> GetColors() const { return colors_.to_host(); }

    PointCloud& Clear() override {
        points_.clear();
        normals_.clear();
        colors_.clear();
        covariances_.clear();
        return *this;
    }
    bool IsEmpty() const override { return !HasPoints(); }
    bool HasPoints() const { return !points_.empty(); }
    bool HasNormals() const { return !points_.empty() && normals_.size() == points_.size(); }
    bool HasColors() const { return !points_.empty() && colors_.size() == points_.size(); }
    bool HasCovariances() const { return !points_.empty() && covariances_.size() == points_.size(); }

    /// pointcloud.cu:205-219 (device reductions; zero vectors for an empty cloud)
    Eigen::Vector3f GetMinBound() const override;
    Eigen::Vector3f GetMaxBound() const override;
    Eigen::Vector3f GetCenter() const override;
    AxisAlignedBoundingBox3 GetAxisAlignedBoundingBox() const override;
    /// pointcloud.cu:225-242
    PointCloud& Translate(const Eigen::Vector3f& translation, bool relative = true) override;
    PointCloud& Scale(const float scale, bool center = true) override;
    PointCloud& Rotate(const Eigen::Matrix3f& R, bool center = true) override;

    /// pointcloud.cu:293-299
    PointCloud& Transform(const Eigen::Matrix4f& transformation) override;
    /// down_sample.cu:170-273
    std::shared_ptr<PointCloud> VoxelDownSample(float voxel_size) const;
    /// down_sample.cu:40-62,110-129: a gather in the order given; invert: the points not named, ascending (a
    /// repeated index counts once).  An index outside [0, size) throws.
    std::shared_ptr<PointCloud> SelectByIndex(const utility::device_vector<size_t>& indices, bool invert = false) const;
    /// down_sample.cu:131-168: the points whose mask entry is set (invert: not set), ascending.  A mask of another
    /// size logs an error and gives an empty cloud, as in the reference.
    std::shared_ptr<PointCloud> SelectByMask(const utility::device_vector<bool>& mask, bool invert = false) const;
    /// down_sample.cu:275-316: points 0, k, 2k, ... (size / k of them); every_k_points == 0 throws
    std::shared_ptr<PointCloud> UniformDownSample(size_t every_k_points) const;
    /// down_sample.cu:317-352: kept iff nb_points + 1 points (itself included) lie within search_radius;
    /// nb_points + 1 <= knn::NUM_MAX_NN.  Returns the kept cloud and their indices, ascending.
    std::tuple<std::shared_ptr<PointCloud>, utility::device_vector<size_t>> RemoveRadiusOutliers(
            size_t nb_points, float search_radius) const;
    /// down_sample.cu:354-438: kept iff 0 < mean squared distance of the nb_neighbors nearest < mean + std_ratio * std
    /// (fp64 statistics, include/mi_icp.h); nb_neighbors <= knn::NUM_MAX_NN.  Returns the kept cloud and their indices.
    std::tuple<std::shared_ptr<PointCloud>, utility::device_vector<size_t>> RemoveStatisticalOutliers(
            size_t nb_neighbors, float std_ratio) const;
    /// pointcloud.cu:40-54,360-385: drops, in place, the points with a NaN (remove_nan) or infinite (remove_infinite)
    /// coordinate, with their normals and colours
    PointCloud& RemoveNoneFinitePoints(bool remove_nan = true, bool remove_infinite = true);
    /// pointcloud.cu:56-106,387-434: every point, normal and colour replaced by the mean of its radius neighbours
    /// (at most num_max_search_points <= knn::NUM_MAX_NN, itself included) weighted with exp(-0.5 d2 / sigma2); normals
    /// are not re-normalised.  Illegal parameters log an error and give an empty cloud, as in the reference.
    std::shared_ptr<PointCloud> GaussianFilter(float search_radius, float sigma2, size_t num_max_search_points = 50);
    /// pointcloud.cu:108-120,436-466: the points with min_bound <= p[axis_no] <= max_bound (a NaN coordinate is kept);
    /// axis_no >= 3 logs an error and gives an empty cloud
    std::shared_ptr<PointCloud> PassThroughFilter(size_t axis_no, float min_bound, float max_bound);
    /// pointcloud.cu:122-139,301-338: num_samples points, each the farthest from those chosen before it; point 0
    /// first, ties to the lowest index (the contract: include/mi_icp.h).  More samples than points logs an error and
    /// gives an empty cloud.
    std::shared_ptr<PointCloud> FarthestPointDownSample(size_t num_samples) const;
    /// pointcloud.cu:340-348: the points inside the closed box; an empty box logs an error and gives an empty cloud
    std::shared_ptr<PointCloud> Crop(const AxisAlignedBoundingBox3& bbox) const;
    /// pointcloud_cluster.cu:109-179: one label per point, its cluster's number or -1 (the contract: include/mi_icp.h);
    /// max_edges <= knn::NUM_MAX_NN.  print_progress is accepted and prints nothing.
    std::unique_ptr<utility::device_vector<int>> ClusterDBSCAN(float eps, size_t min_points, bool print_progress = false,
                                                               size_t max_edges = knn::NUM_MAX_NN) const;
    /// segmentation.cu:187-268: RANSAC over planes through three points, the best one refit to its inliers (the
    /// contract: include/mi_icp.h).  Returns (a, b, c, d) of a x + b y + c z + d = 0 and the inliers' indices, ascending.
    /// The seed is taken from rand(), as the reference takes its seeds: std::srand governs the result.
    std::tuple<Eigen::Vector4f, utility::device_vector<size_t>> SegmentPlane(float distance_threshold = 0.01,
                                                                             size_t ransac_n = 3,
                                                                             size_t num_iterations = 100) const;
    /// estimate_normals.cu:82-127 (KNN or radius search parameter; up to knn::NUM_MAX_NN neighbours)
    bool EstimateNormals(const knn::KDTreeSearchParam& search_param = knn::KDTreeSearchParamKNN());

    /// pointcloud_factory.cu:329-351 (float or uint16 depth)
    static std::shared_ptr<PointCloud> CreateFromDepthImage(const Image& depth,
                                                            const camera::PinholeCameraIntrinsic& intrinsic,
                                                            const Eigen::Matrix4f& extrinsic = Eigen::Matrix4f::Identity(),
                                                            float depth_scale = 1000.0, float depth_trunc = 1000.0,
                                                            int stride = 1);
    /// pointcloud_factory.cu:353-376 (colour uint8 x 3 or float x 1; an empty colour image
    /// gives a cloud without colours)
    static std::shared_ptr<PointCloud> CreateFromRGBDImage(const RGBDImage& image,
                                                           const camera::PinholeCameraIntrinsic& intrinsic,
                                                           const Eigen::Matrix4f& extrinsic = Eigen::Matrix4f::Identity(),
                                                           bool project_valid_depth_only = true,
                                                           float depth_cutoff = -1.0f, bool compute_normals = false);
    /// pointcloud_factory.cu:432-482: one point and one colour per pixel of an 8-bit disparity image (as
    /// imageproc::SemiGlobalMatching makes it) in raster order, none left out; `color` has the same size and 3 channels
    /// of 1 or 2 bytes (else "[PointCloud::CreateFromDisparity] Unsupported image format." and an empty cloud).  A
    /// disparity at which w = 0 gives non-finite coordinates: RemoveNoneFinitePoints takes them out.  The arithmetic:
    /// include/mi_icp.h "stereo".
    static std::shared_ptr<PointCloud> CreateFromDisparity(const Image& disp, const Image& color,
                                                           const camera::PinholeCameraIntrinsic& left_intrinsic,
                                                           const camera::PinholeCameraIntrinsic& right_intrinsic,
                                                           float baseline);
    /// pointcloud_factory.cu:418-430: the centres of the grid's occupied voxels, every colour (0, 0, 1)
    static std::shared_ptr<PointCloud> CreateFromOccupancyGrid(const OccupancyGrid& occgrid);
    /// pointcloud_factory.cu:375-420: the LIVE scans' readings inside [min_range, max_range] as points in the frame of their
    /// origins, oldest scan first, non-finite points removed; intensities become grey colours (include/mi_icp.h "laserscan")
    static std::shared_ptr<PointCloud> CreateFromLaserScanBuffer(const LaserScanBuffer& scan, float min_range, float max_range);

public:
    utility::device_vector<Eigen::Vector3f> points_;
    utility::device_vector<Eigen::Vector3f> normals_;
    utility::device_vector<Eigen::Vector3f> colors_;
    utility::device_vector<Eigen::Matrix3f> covariances_;
};

}  // namespace geometry
}  // namespace cupoch
