// cupoch/geometry/distancetransform.h -- geometry::DistanceTransform and geometry::DistanceVoxel (reference:
// geometry/distancetransform.h:30-78 with the members of geometry/densegrid.h it uses) over mi_icp_dt_*
// (include/mi_icp.h has the contract).  The cells live in the engine's context, one word per cell (the nearest site's
// index) in two planes, made on first use; GetVoxels() reads the plane back as DistanceVoxel records instead of a public
// voxels_ vector.  The public members are read when a call is made, as in the reference.
// Every compute REPLACES the site set; cells outside the grid are dropped; any resolution in [2, 1024]; ComputeEDT and
// ComputeVoronoiDiagram are one call (the distance is derived from the nearest index when it is read); a transform
// without sites reads +inf; queries follow DenseGrid::GetVoxelIndex and give NaN outside the grid; state_ keeps only the
// not-a-site bit.  Copy construction is deleted, as OccupancyGrid's is here.  Deviations: DESIGN.md section 6.
// Not built: the collision, planning and visualisation consumers of a transform.
#pragma once
#include <limits>
#include <memory>
#include <tuple>
#include <vector>

#include "cupoch/geometry/pointcloud.h"

struct mi_icp_dt;

namespace cupoch {
namespace geometry {

class VoxelGrid;
class OccupancyGrid;

class DistanceVoxel {
public:
    enum State {
        HasNext = 1,  // (the reference's working bit; never set here)
        NotSite = 1 << 1,
    };
    DistanceVoxel() {}
    DistanceVoxel(const Eigen::Vector3ui16& nearest_index, unsigned char state) : nearest_index_(nearest_index), state_(state) {}

    /// no site has been given: nearest_index_ is (65535, 65535, 65535) and distance_ +inf
    bool IsNotSite() const { return state_ & NotSite; }

public:
    Eigen::Vector3ui16 nearest_index_ = Eigen::Vector3ui16::Zero();
    unsigned char state_ = NotSite;
    float distance_ = 0;
};

class DistanceTransform : public GeometryBase3D {
public:
    DistanceTransform();
    DistanceTransform(float voxel_size, size_t resolution, const Eigen::Vector3f& origin = Eigen::Vector3f::Zero());
    ~DistanceTransform() override;
    DistanceTransform(const DistanceTransform&) = delete;  // (the reference copies the voxels; not provided)
    DistanceTransform& operator=(const DistanceTransform&) = delete;

    /// no sites; size and memory stay
    DistanceTransform& Clear() override;
    bool IsEmpty() const override { return false; }
    Eigen::Vector3f GetMinBound() const override;
    Eigen::Vector3f GetMaxBound() const override;
    Eigen::Vector3f GetCenter() const override { return origin_; }
    AxisAlignedBoundingBox3 GetAxisAlignedBoundingBox() const override;
    /// not defined for a grid: logs an error and changes nothing, as in the reference
    DistanceTransform& Transform(const Eigen::Matrix4f& transformation) override;
    DistanceTransform& Rotate(const Eigen::Matrix3f& R, bool center = true) override;
    DistanceTransform& Translate(const Eigen::Vector3f& translation, bool relative = true) override;
    DistanceTransform& Scale(const float scale, bool center = true) override;

    DistanceTransform& Reconstruct(float voxel_size, size_t resolution);

    /// grid indices in [0, resolution)^3; those outside are dropped
    DistanceTransform& ComputeEDT(const utility::device_vector<Eigen::Vector3i>& points);
    /// a voxel size other than the grid's logs an error and changes nothing
    DistanceTransform& ComputeEDT(const VoxelGrid& voxelgrid);
    DistanceTransform& ComputeVoronoiDiagram(const utility::device_vector<Eigen::Vector3i>& points);
    DistanceTransform& ComputeVoronoiDiagram(const VoxelGrid& voxelgrid);

    /// NaN for a point outside the grid on any axis, +inf without a site
    float GetDistance(const Eigen::Vector3f& query) const;
    std::unique_ptr<utility::device_vector<float>> GetDistances(const utility::device_vector<Eigen::Vector3f>& queries) const;
    /// (inside the grid, the cell of the point)
    std::tuple<bool, DistanceVoxel> GetVoxel(const Eigen::Vector3f& point) const;
    /// the whole plane: resolution^3 records, indexed (x*res + y)*res + z
    std::vector<DistanceVoxel> GetVoxels() const;

    /// the COMPUTED transform of the occupied voxels, with the grid's voxel size, resolution and origin
    static std::shared_ptr<DistanceTransform> CreateFromOccupancyGrid(const OccupancyGrid& input);

public:
    float voxel_size_ = 0.05f;
    int resolution_ = 512;
    Eigen::Vector3f origin_ = Eigen::Vector3f::Zero();

private:
    mi_icp_dt* Handle() const;
    mutable mi_icp_dt* dt_ = nullptr;
    mutable int made_resolution_ = 0;
};

}  // namespace geometry
}  // namespace cupoch
