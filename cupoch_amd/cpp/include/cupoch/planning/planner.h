// cupoch/planning/planner.h -- planning::PlannerBase, Pos3DPlanner and Path (reference: planning/planner.h).  FindPath
// copies the roadmap, adds the start (lazily) and the goal as nodes n and n + 1, each joined to every node nearer than
// max_edge_distance_, prices the edges that collide with an obstacle at margin object_radius_ at +inf
// (collision::ComputeIntersection, whose segment predicate is symmetric in the end points: both directions of an edge
// go together) and searches n -> n + 1 (geometry::Graph<3>::DijkstraPath).  Obstacles: VoxelGrid and OccupancyGrid.
#pragma once
#include <memory>
#include <vector>

#include "cupoch/geometry/graph.h"

namespace cupoch {
namespace planning {

typedef std::vector<Eigen::Vector3f> Path;

class PlannerBase {
public:
    PlannerBase() {}
    virtual ~PlannerBase() {}
    PlannerBase(const PlannerBase& other) : obstacles_(other.obstacles_) {}
    virtual PlannerBase& AddObstacle(const std::shared_ptr<geometry::Geometry>& obstacle) {
        obstacles_.push_back(obstacle);
        return *this;
    }
    virtual std::shared_ptr<Path> FindPath(const Eigen::Vector3f& start, const Eigen::Vector3f& goal) const = 0;

public:
    std::vector<std::shared_ptr<geometry::Geometry>> obstacles_;
};

class Pos3DPlanner : public PlannerBase {
public:
    Pos3DPlanner(const geometry::Graph<3>& graph, float object_radius = 0.1, float max_edge_distance = 1.0);
    ~Pos3DPlanner() override;
    Pos3DPlanner(const Pos3DPlanner& other);

    Pos3DPlanner& UpdateGraph();
    std::shared_ptr<Path> FindPath(const Eigen::Vector3f& start, const Eigen::Vector3f& goal) const override;
    const geometry::Graph<3>& GetGraph() const { return graph_; }

private:
    void RemoveCollisionEdges(geometry::Graph<3>& graph) const;

public:
    geometry::Graph<3> graph_;
    float object_radius_;
    float max_edge_distance_;
};

}  // namespace planning
}  // namespace cupoch
