// cupoch/geometry/lineset.h -- geometry::LineSet<3> (reference: geometry/lineset.h): points, lines (pairs of point
// indices) and optional colours, one per line, on the device.  The bounds and the moves are the point cloud's, through
// the same entry points (mi_icp_compute_bounds, mi_icp_affine, mi_icp_transform).  Its consumer here is
// collision::ComputeIntersection (collision/collision.h); geometry::Graph<3> (geometry/graph.h) derives from it.
// Not built: the factories from triangle meshes, oriented boxes and clouds with correspondences, other dimensions,
// file I/O, visualisation.
#pragma once
#include <memory>
#include <utility>

#include "cupoch/geometry/pointcloud.h"

namespace cupoch {
namespace geometry {

template <int Dim>
class LineSet;

template <>
class LineSet<3> : public GeometryBase3D {
public:
    LineSet();
    LineSet(const utility::device_vector<Eigen::Vector3f>& points, const utility::device_vector<Eigen::Vector2i>& lines);
    LineSet(const thrust::host_vector<Eigen::Vector3f>& points, const thrust::host_vector<Eigen::Vector2i>& lines);
    ~LineSet() override;

    void SetPoints(const thrust::host_vector<Eigen::Vector3f>& points) { points_ = points; }
    thrust::host_vector<Eigen::Vector3f> GetPoints() const { return points_.to_host(); }
    void SetLines(const thrust::host_vector<Eigen::Vector2i>& lines) { lines_ = lines; }
    thrust::host_vector<Eigen::Vector2i> GetLines() const { return lines_.to_host(); }
    void SetColors(const thrust::host_vector<Eigen::Vector3f>& colors) { colors_ = colors; }
    thrust::host_vector<Eigen::Vector3f> GetColors() const { return colors_.to_host(); }

    LineSet& Clear() override;
    bool IsEmpty() const override { return !HasPoints(); }
    Eigen::Vector3f GetMinBound() const override;
    Eigen::Vector3f GetMaxBound() const override;
    Eigen::Vector3f GetCenter() const override;
    AxisAlignedBoundingBox3 GetAxisAlignedBoundingBox() const override;
    LineSet& Transform(const Eigen::Matrix4f& transformation) override;
    LineSet& Translate(const Eigen::Vector3f& translation, bool relative = true) override;
    LineSet& Scale(const float scale, bool center = true) override;
    LineSet& Rotate(const Eigen::Matrix3f& R, bool center = true) override;

    bool HasPoints() const { return points_.size() > 0; }
    bool HasLines() const { return HasPoints() && lines_.size() > 0; }
    bool HasColors() const { return HasLines() && colors_.size() == lines_.size(); }
    /// the two end points of a line; zeros for an index (of the line, or of one of its points) out of range
    std::pair<Eigen::Vector3f, Eigen::Vector3f> GetLineCoordinate(size_t line_index) const;
    LineSet& PaintUniformColor(const Eigen::Vector3f& color);

    /// the twelve edges of a box
    static std::shared_ptr<LineSet<3>> CreateFromAxisAlignedBoundingBox(const AxisAlignedBoundingBox3& box);

protected:
    explicit LineSet(GeometryType type);  // (a subclass with a type of its own: geometry::Graph<3>)

public:
    utility::device_vector<Eigen::Vector3f> points_;
    utility::device_vector<Eigen::Vector2i> lines_;
    utility::device_vector<Eigen::Vector3f> colors_;
};

}  // namespace geometry
}  // namespace cupoch
