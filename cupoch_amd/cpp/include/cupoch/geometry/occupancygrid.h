// cupoch/geometry/occupancygrid.h -- geometry::OccupancyGrid and geometry::OccupancyVoxel (reference:
// geometry/occupancygrid.h:31-142 with the members of geometry/densegrid.h it uses) over mi_icp_occgrid_*
// (include/mi_icp.h has the numeric contract).  The voxels live in the engine's context as one plane of log-odds,
// made on first use; GetVoxels() reads the plane back instead of a public voxels_ vector, and the extractions return
// OccupancyVoxel records whose grid_index_ is the voxel's position and whose colour is the constant (0, 0, 1).
// The public members are read when a call is made, as in the reference; min_bound_ / max_bound_ are refreshed by every
// call that changes them.  Clear() leaves a usable grid (every voxel unknown), where the reference's leaves none.
// Not built: CreateFromVoxelGrid (VoxelGrid::CreateFromOccupancyGrid takes the occupied space out:
// geometry/voxelgrid.h; DistanceTransform::CreateFromOccupancyGrid its distance field: geometry/distancetransform.h;
// collisions: collision/collision.h).
#pragma once
#include <limits>
#include <memory>
#include <tuple>
#include <vector>

#include "cupoch/geometry/pointcloud.h"

struct mi_icp_occgrid;

namespace cupoch {
namespace geometry {

class OccupancyVoxel {
public:
    OccupancyVoxel() {}
    OccupancyVoxel(const Eigen::Vector3i& grid_index) : grid_index_(Cast(grid_index)) {}
    OccupancyVoxel(const Eigen::Vector3i& grid_index, float prob_log) : grid_index_(Cast(grid_index)), prob_log_(prob_log) {}
    OccupancyVoxel(const Eigen::Vector3i& grid_index, float prob_log, const Eigen::Vector3f& color)
        : grid_index_(Cast(grid_index)), color_(color), prob_log_(prob_log) {}

public:
    Eigen::Vector3ui16 grid_index_ = Eigen::Vector3ui16::Zero();
    Eigen::Vector3f color_ = Eigen::Vector3f(0.0f, 0.0f, 1.0f);
    float prob_log_ = std::numeric_limits<float>::quiet_NaN();

private:
    static Eigen::Vector3ui16 Cast(const Eigen::Vector3i& v) {
        return Eigen::Vector3ui16((unsigned short)v[0], (unsigned short)v[1], (unsigned short)v[2]);
    }
};

class OccupancyGrid : public GeometryBase3D {
public:
    OccupancyGrid();
    OccupancyGrid(float voxel_size, size_t resolution = 512, const Eigen::Vector3f& origin = Eigen::Vector3f::Zero());
    ~OccupancyGrid() override;
    OccupancyGrid(const OccupancyGrid&) = delete;  // (the reference copies the voxels; not provided)
    OccupancyGrid& operator=(const OccupancyGrid&) = delete;

    /// every voxel unknown, the bounds back to the centre; size and memory stay
    OccupancyGrid& Clear() override;
    bool IsEmpty() const override { return false; }
    Eigen::Vector3f GetMinBound() const override;
    Eigen::Vector3f GetMaxBound() const override;
    Eigen::Vector3f GetCenter() const override { return origin_; }
    AxisAlignedBoundingBox3 GetAxisAlignedBoundingBox() const override;
    /// not defined for a grid: logs an error and changes nothing, as in the reference
    OccupancyGrid& Transform(const Eigen::Matrix4f& transformation) override;
    OccupancyGrid& Rotate(const Eigen::Matrix3f& R, bool center = true) override;
    OccupancyGrid& Translate(const Eigen::Vector3f& translation, bool relative = true) override;
    OccupancyGrid& Scale(const float scale, bool center = true) override;

    bool HasVoxels() const { return true; }
    bool HasColors() const { return true; }
    /// the voxel of a point is floor((point - origin) / voxel_size) + resolution / 2 per axis; a point outside the grid
    /// on any axis is unknown
    bool IsOccupied(const Eigen::Vector3f& point) const;
    bool IsUnknown(const Eigen::Vector3f& point) const;
    std::tuple<bool, OccupancyVoxel> GetVoxel(const Eigen::Vector3f& point) const;
    /// batched: the log-odds of every point's voxel, NaN for unknown or outside
    utility::device_vector<float> GetProbLog(const utility::device_vector<Eigen::Vector3f>& points) const;
    /// the voxels of the box [min_bound_, max_bound_], ascending in linear index (x*res + y)*res + z
    std::shared_ptr<std::vector<OccupancyVoxel>> ExtractKnownVoxels() const;
    std::shared_ptr<std::vector<OccupancyVoxel>> ExtractFreeVoxels() const;
    std::shared_ptr<std::vector<OccupancyVoxel>> ExtractOccupiedVoxels() const;

    OccupancyGrid& Reconstruct(float voxel_size, int resolution);
    OccupancyGrid& SetFreeArea(const Eigen::Vector3f& min_bound, const Eigen::Vector3f& max_bound);
    OccupancyGrid& Insert(const utility::device_vector<Eigen::Vector3f>& points, const Eigen::Vector3f& viewpoint,
                          float max_range = -1.0f);
    OccupancyGrid& Insert(const thrust::host_vector<Eigen::Vector3f>& points, const Eigen::Vector3f& viewpoint,
                          float max_range = -1.0f);
    OccupancyGrid& Insert(const PointCloud& pointcloud, const Eigen::Vector3f& viewpoint, float max_range = -1.0f);
    /// an index outside the grid logs an error and changes nothing; a voxel listed twice is updated once
    OccupancyGrid& AddVoxel(const Eigen::Vector3i& voxel, bool occupied = false);
    OccupancyGrid& AddVoxels(const utility::device_vector<Eigen::Vector3i>& voxels, bool occupied = false);

    /// the whole plane: resolution^3 log-odds, NaN unknown
    std::vector<float> GetVoxels() const;
    /// the engine's handle (made on first use; a changed resolution_ rebuilds the grid), for PointCloud's factory
    mi_icp_occgrid* Handle() const;

public:
    float voxel_size_ = 0.05f;
    int resolution_ = 512;
    Eigen::Vector3f origin_ = Eigen::Vector3f::Zero();
    /// inclusive voxel indices, both (h, h, h) at first (int where the reference has unsigned short: a SetFreeArea
    /// beside the grid leaves min > max on an axis, a negative max among them)
    mutable Eigen::Vector3i min_bound_;
    mutable Eigen::Vector3i max_bound_;
    float clamping_thres_min_ = -2.0f;
    float clamping_thres_max_ = 3.5f;
    float prob_hit_log_ = 0.85f;
    float prob_miss_log_ = -0.4f;
    float occ_prob_thres_log_ = 0.0f;
    bool visualize_free_area_ = true;

private:
    std::shared_ptr<std::vector<OccupancyVoxel>> Extract(int which) const;
    void RefreshBounds() const;
    mutable mi_icp_occgrid* grid_ = nullptr;
    mutable int made_resolution_ = 0;
};

}  // namespace geometry
}  // namespace cupoch
