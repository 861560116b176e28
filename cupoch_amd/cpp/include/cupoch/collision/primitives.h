// cupoch/collision/primitives.h -- collision::Primitive, Box, Sphere, Capsule, Cylinder, Mesh, PrimitivePack and
// PrimitiveArray (reference: collision/primitives.h) as host values; a query copies the array's 80-byte records
// (mi_icp_primitive) to the device.  include/mi_icp.h has the numeric contract, the bounding boxes included: a box's is
// |rot| * half lengths (the reference's |rot * half| does not contain a rotated box) and a cylinder's max bound takes max.
// Not built: CreateVoxelGridWithSweeping, CreateTriangleMesh, Mesh primitives (a Mesh never collides).
#pragma once
#include <memory>
#include <vector>

#include "cupoch/geometry/pointcloud.h"

namespace cupoch {
namespace geometry {
class VoxelGrid;
}

namespace collision {

class Primitive {
public:
    enum class PrimitiveType { Unspecified = 0, Box = 1, Sphere = 2, Capsule = 3, Cylinder = 4, Mesh = 5 };
    Primitive() {}
    Primitive(PrimitiveType type) : type_(type) {}
    Primitive(PrimitiveType type, const Eigen::Matrix4f& transform) : type_(type), transform_(transform) {}
    virtual ~Primitive() {}

    /// Box, Sphere, Capsule and Cylinder by the rules of include/mi_icp.h; zeros for the other types
    geometry::AxisAlignedBoundingBox3 GetAxisAlignedBoundingBox() const;
    /// lengths, or radius and height: the three floats of the C record
    virtual Eigen::Vector3f Parameters() const { return Eigen::Vector3f::Zero(); }

    PrimitiveType type_ = PrimitiveType::Unspecified;
    Eigen::Matrix4f transform_ = Eigen::Matrix4f::Identity();
};

class Box : public Primitive {
public:
    Box() : Primitive(PrimitiveType::Box) {}
    Box(const Eigen::Vector3f& lengths) : Primitive(PrimitiveType::Box), lengths_(lengths) {}
    Box(const Eigen::Vector3f& lengths, const Eigen::Matrix4f& transform) : Primitive(PrimitiveType::Box, transform), lengths_(lengths) {}
    Eigen::Vector3f Parameters() const override { return lengths_; }
    Eigen::Vector3f lengths_ = Eigen::Vector3f::Zero();
};

class Sphere : public Primitive {
public:
    Sphere() : Primitive(PrimitiveType::Sphere) {}
    Sphere(float radius) : Primitive(PrimitiveType::Sphere), radius_(radius) {}
    Sphere(float radius, const Eigen::Vector3f& center) : Primitive(PrimitiveType::Sphere), radius_(radius) {
        for (int k = 0; k < 3; ++k) transform_(k, 3) = center(k);
    }
    Eigen::Vector3f Parameters() const override { return Eigen::Vector3f(radius_, 0.0f, 0.0f); }
    float radius_ = 0.0f;
};

class Capsule : public Primitive {
public:
    Capsule() : Primitive(PrimitiveType::Capsule) {}
    Capsule(float radius, float height) : Primitive(PrimitiveType::Capsule), radius_(radius), height_(height) {}
    Capsule(float radius, float height, const Eigen::Matrix4f& transform)
        : Primitive(PrimitiveType::Capsule, transform), radius_(radius), height_(height) {}
    Eigen::Vector3f Parameters() const override { return Eigen::Vector3f(radius_, height_, 0.0f); }
    float radius_ = 0.0f;
    float height_ = 0.0f;
};

class Cylinder : public Primitive {
public:
    Cylinder() : Primitive(PrimitiveType::Cylinder) {}
    Cylinder(float radius, float height) : Primitive(PrimitiveType::Cylinder), radius_(radius), height_(height) {}
    Cylinder(float radius, float height, const Eigen::Matrix4f& transform)
        : Primitive(PrimitiveType::Cylinder, transform), radius_(radius), height_(height) {}
    Eigen::Vector3f Parameters() const override { return Eigen::Vector3f(radius_, height_, 0.0f); }
    float radius_ = 0.0f;
    float height_ = 0.0f;
};

class Mesh : public Primitive {
public:
    Mesh() : Primitive(PrimitiveType::Mesh) {}
    Mesh(const Eigen::Matrix4f& transform) : Primitive(PrimitiveType::Mesh, transform) {}
};

/// one primitive of any type, as the array holds it: the C record's fields
struct PrimitivePack {
    PrimitivePack() {}
    PrimitivePack(const Primitive& p) : type_(p.type_), transform_(p.transform_), parameters_(p.Parameters()) {}
    Primitive::PrimitiveType type_ = Primitive::PrimitiveType::Unspecified;
    Eigen::Matrix4f transform_ = Eigen::Matrix4f::Identity();
    Eigen::Vector3f parameters_ = Eigen::Vector3f::Zero();
};
static_assert(sizeof(PrimitivePack) == 80, "a PrimitivePack is the 80-byte record of include/mi_icp.h");

typedef std::vector<PrimitivePack> PrimitiveArray;

/// the cells of a lattice around the primitive that it collides with; voxel_size <= 0 or a type other than Box,
/// Sphere, Capsule logs an error and returns an empty grid
std::shared_ptr<geometry::VoxelGrid> CreateVoxelGrid(const Primitive& primitive, float voxel_size);

}  // namespace collision
}  // namespace cupoch
