// cupoch/collision/collision.h -- collision::CollisionResult, ComputeIntersection and Intersection<TargetT> (reference:
// collision/collision.h) over mi_icp_collision_compute (include/mi_icp.h has the contract: the predicates, which side
// is enumerated, the smallest index of the other side, ascending pairs).  Column 0 of a pair indexes the first
// argument, column 1 the second, for every overload.
// Not built: Primitives x Primitives (declared, never defined in the reference), a DistanceTransform as a target.
#pragma once
#include <memory>

#include "cupoch/collision/primitives.h"
#include "cupoch/geometry/lineset.h"
#include "cupoch/geometry/occupancygrid.h"
#include "cupoch/geometry/voxelgrid.h"

namespace cupoch {
namespace collision {

struct CollisionResult {
    enum class CollisionType { Unspecified = 0, Primitives = 1, VoxelGrid = 2, OccupancyGrid = 3, LineSet = 4 };
    CollisionType first_ = CollisionType::Unspecified;
    CollisionType second_ = CollisionType::Unspecified;
    utility::device_vector<Eigen::Vector2i> collision_index_pairs_;

    CollisionResult() {}
    CollisionResult(CollisionType first, CollisionType second) : first_(first), second_(second) {}
    CollisionResult(CollisionType first, CollisionType second, const utility::device_vector<Eigen::Vector2i>& collision_index_pairs)
        : first_(first), second_(second), collision_index_pairs_(collision_index_pairs) {}

    bool IsCollided() const { return !collision_index_pairs_.empty(); }
    thrust::host_vector<Eigen::Vector2i> GetCollisionIndexPairs() const { return collision_index_pairs_.to_host(); }
    utility::device_vector<size_t> GetFirstCollisionIndices() const;
    utility::device_vector<size_t> GetSecondCollisionIndices() const;
};

std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::VoxelGrid& voxelgrid1, const geometry::VoxelGrid& voxelgrid2, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::VoxelGrid& voxelgrid, const geometry::LineSet<3>& lineset, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::LineSet<3>& lineset, const geometry::VoxelGrid& voxelgrid, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::VoxelGrid& voxelgrid, const geometry::OccupancyGrid& occgrid, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::OccupancyGrid& occgrid, const geometry::VoxelGrid& voxelgrid, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::LineSet<3>& lineset, const geometry::OccupancyGrid& occgrid, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::OccupancyGrid& occgrid, const geometry::LineSet<3>& lineset, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const PrimitiveArray& primitives, const geometry::VoxelGrid& voxelgrid, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::VoxelGrid& voxelgrid, const PrimitiveArray& primitives, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const PrimitiveArray& primitives, const geometry::OccupancyGrid& occgrid, float margin = 0.0f);
std::shared_ptr<CollisionResult> ComputeIntersection(const geometry::OccupancyGrid& occgrid, const PrimitiveArray& primitives, float margin = 0.0f);

/// A target kept for several queries.  A VoxelGrid whose keys are not known to ascend is sorted once here, with the
/// index every key has in the target, so that its queries do not sort again; every other target is used as it is.
/// Compute(query) is ComputeIntersection(target, query): column 0 indexes the target.
template <typename TargetT>
class Intersection {
public:
    Intersection(const TargetT& target) : target_(target) { Construct(); }
    template <typename QueryT>
    std::shared_ptr<CollisionResult> Compute(const QueryT& query, float margin = 0.0f) const;

private:
    void Construct();

public:
    const TargetT& target_;
    utility::device_vector<Eigen::Vector3i> sorted_keys_;  // VoxelGrid targets that came unsorted: the ascending keys ...
    utility::device_vector<int> sorted_index_;             // ... and each one's index in target_
};

}  // namespace collision
}  // namespace cupoch
