// cupoch/geometry/voxelgrid.h -- geometry::Voxel and geometry::VoxelGrid (reference: geometry/voxelgrid.h:48-214) over
// mi_icp_voxelgrid_* (include/mi_icp.h has the numeric contract).  The public members are the reference's:
// voxels_keys_ and voxels_values_ on the device, voxel_size_, origin_.  The engine takes keys and colours as two arrays,
// so a call that reads or replaces the voxels moves the colours out of / into voxels_values_ with strided device copies.
// Every factory, operator+= and AddVoxel[s] leave the keys distinct and ascending (x most significant).  LogError logs
// and returns, as in the reference.  Deviations from the reference: DESIGN.md section 6.
// Not built: CreateFromTriangleMesh[WithinBounds] (no TriangleMesh here), GetOrientedBoundingBox, VoxelGrid file I/O,
// visualisation.  (The distance field of a grid: geometry/distancetransform.h; collisions: collision/collision.h.)
#pragma once
#include <array>
#include <memory>
#include <utility>
#include <vector>

#include "cupoch/camera/pinhole_camera_parameters.h"
#include "cupoch/geometry/image.h"
#include "cupoch/geometry/pointcloud.h"

namespace cupoch {
namespace geometry {

class OccupancyGrid;

class Voxel {
public:
    Voxel() {}
    Voxel(const Eigen::Vector3i& grid_index) : grid_index_(grid_index) {}
    Voxel(const Eigen::Vector3f& color) : color_(color) {}
    Voxel(const Eigen::Vector3i& grid_index, const Eigen::Vector3f& color) : grid_index_(grid_index), color_(color) {}

public:
    Eigen::Vector3i grid_index_ = Eigen::Vector3i(0, 0, 0);
    Eigen::Vector3f color_ = Eigen::Vector3f(1.0f, 1.0f, 1.0f);
};
static_assert(sizeof(Voxel) == 24, "a Voxel is its index and its colour, packed");

class VoxelGrid : public GeometryBase3D {
public:
    VoxelGrid();
    VoxelGrid(const VoxelGrid& src_voxel_grid);
    VoxelGrid& operator=(const VoxelGrid&) = default;
    ~VoxelGrid() override;

    std::pair<thrust::host_vector<Eigen::Vector3i>, thrust::host_vector<Voxel>> GetVoxels() const;
    void SetVoxels(const thrust::host_vector<Eigen::Vector3i>& voxels_keys, const thrust::host_vector<Voxel>& voxels_values);

    VoxelGrid& Clear() override;
    bool IsEmpty() const override;
    Eigen::Vector3f GetMinBound() const override;
    Eigen::Vector3f GetMaxBound() const override;
    /// the double-precision mean of the voxel centres, rounded once (the reference sums in fp32)
    Eigen::Vector3f GetCenter() const override;
    AxisAlignedBoundingBox3 GetAxisAlignedBoundingBox() const override;
    /// not defined for a grid: logs an error and changes nothing, as in the reference
    VoxelGrid& Transform(const Eigen::Matrix4f& transformation) override;
    VoxelGrid& Rotate(const Eigen::Matrix3f& R, bool center = true) override;
    /// these touch only the origin and the voxel size
    VoxelGrid& Translate(const Eigen::Vector3f& translation, bool relative = true) override;
    VoxelGrid& Scale(const float scale, bool center = true) override;

    /// one voxel per key, ascending; a key both grids hold gets the fp32 sum of its colours over their number.  A
    /// differing voxel_size_ or origin_ logs an error (and merges, as the reference does)
    VoxelGrid& operator+=(const VoxelGrid& voxelgrid);
    VoxelGrid operator+(const VoxelGrid& voxelgrid) const;

    bool HasVoxels() const { return voxels_keys_.size() > 0; }
    bool HasColors() const { return true; }  // by default the colours are (1, 1, 1)
    /// the keys are known to ascend (every producer here; not after SetVoxels / SelectByIndex)
    bool KeysSorted() const { return sorted_; }
    Eigen::Vector3i GetVoxel(const Eigen::Vector3f& point) const;
    /// the zero vector when the grid has no such voxel
    Eigen::Vector3f GetVoxelCenterCoordinate(const Eigen::Vector3i& idx) const;
    std::array<Eigen::Vector3f, 8> GetVoxelBoundingPoints(const Eigen::Vector3i& index) const;

    /// an existing voxel stays as it is; among added voxels of one index the first listed stays
    void AddVoxel(const Voxel& voxel);
    void AddVoxels(const utility::device_vector<Voxel>& voxels);
    void AddVoxels(const thrust::host_vector<Voxel>& voxels);

    VoxelGrid& PaintUniformColor(const Eigen::Vector3f& color);
    /// an index outside the grid logs an error and paints nothing
    VoxelGrid& PaintIndexedColor(const utility::device_vector<size_t>& indices, const Eigen::Vector3f& color);

    /// one binary search per query (the grid is sorted first when a SetVoxels or SelectByIndex left it in another order)
    thrust::host_vector<bool> CheckIfIncluded(const thrust::host_vector<Eigen::Vector3f>& queries);

    VoxelGrid& CarveDepthMap(const Image& depth_map, const camera::PinholeCameraParameters& camera_parameter,
                             bool keep_voxels_outside_image);
    VoxelGrid& CarveSilhouette(const Image& silhouette_mask, const camera::PinholeCameraParameters& camera_parameter,
                               bool keep_voxels_outside_image);

    /// an index out of range logs an error and returns an empty grid; invert treats a repeated index once
    std::shared_ptr<VoxelGrid> SelectByIndex(const utility::device_vector<size_t>& indices, bool invert = false);

    static std::shared_ptr<VoxelGrid> CreateDense(const Eigen::Vector3f& origin, float voxel_size, float width, float height,
                                                  float depth);
    static std::shared_ptr<VoxelGrid> CreateFromPointCloud(const PointCloud& input, float voxel_size);
    static std::shared_ptr<VoxelGrid> CreateFromPointCloudWithinBounds(const PointCloud& input, float voxel_size,
                                                                      const Eigen::Vector3f& min_bound,
                                                                      const Eigen::Vector3f& max_bound);
    /// the occupied voxels' grid indices as keys (already ascending), every colour (0, 0, 1)
    static std::shared_ptr<VoxelGrid> CreateFromOccupancyGrid(const OccupancyGrid& input);

public:
    float voxel_size_ = 0.0f;
    Eigen::Vector3f origin_ = Eigen::Vector3f::Zero();
    utility::device_vector<Eigen::Vector3i> voxels_keys_;
    utility::device_vector<Voxel> voxels_values_;

private:
    bool sorted_ = true;  // the keys are known to ascend (every producer here; not after SetVoxels / SelectByIndex)
};

}  // namespace geometry
}  // namespace cupoch
