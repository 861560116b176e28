// geometry::Graph<3> and planning::Pos3DPlanner through the C++ surface, with the reference's signatures: the
// reference's unit tests (src/tests/geometry/graph.cpp, src/tests/planning/planner.cpp), the zero-weight pair that
// traps the plain predecessor rule, and the wall with a window.  argv[1]: a directory holding wall.i32 and closed.i32
// (raw int32 [m][3] voxel keys) and scene.txt (voxel_size, object_radius, max_edge_distance, start, goal); the paths go
// there as path.f32 / path_closed.f32 / path_free.f32, the updated graph's weights as weights.f32.  Prints one JSON
// line; tests/test_gpu_graph_cpp.py compiles and runs it and holds the output to tests/graph_exact.py.
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

template <class T>
static std::vector<T> ReadRaw(const std::string& path) {
    std::vector<T> v;
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread((void*)v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}

static bool WriteRaw(const std::string& path, const void* p, size_t bytes) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

static std::shared_ptr<geometry::VoxelGrid> Wall(const std::vector<Eigen::Vector3i>& keys, float vs) {
    auto g = std::make_shared<geometry::VoxelGrid>();
    g->voxel_size_ = vs;
    g->origin_ = Eigen::Vector3f::Zero();
    std::vector<geometry::Voxel> values;
    for (const Eigen::Vector3i& k : keys) values.push_back(geometry::Voxel(k));
    g->AddVoxels(values);
    return g;
}

static void PrintInts(const char* name, const std::vector<int>& v) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("], ");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    float vs, radius, reach, s[3], g[3];
    {
        std::FILE* f = std::fopen((dir + "/scene.txt").c_str(), "r");
        if (!f || std::fscanf(f, "%f %f %f %f %f %f %f %f %f", &vs, &radius, &reach, &s[0], &s[1], &s[2], &g[0], &g[1], &g[2]) != 9) return 2;
        std::fclose(f);
    }
    std::printf("{");

    // ---- src/tests/geometry/graph.cpp
    geometry::Graph<3> empty;
    const bool ctor = empty.GetGeometryType() == geometry::Geometry::GeometryType::Graph && empty.Dimension() == 3 && empty.IsEmpty() &&
                      !empty.HasLines() && !empty.HasWeights() && !empty.IsConstructed() && empty.edge_index_offsets_.size() == 0;
    geometry::Graph<3> gp;
    gp.SetPoints({{0.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {1.0f, 1.0f, 0.0f}, {2.0f, 2.0f, 0.0f}});
    gp.AddEdge({0, 1});
    gp.AddEdge({0, 2}, 2.0);
    gp.AddEdge({1, 3});
    gp.AddEdge({2, 3});
    gp.AddEdge({3, 4});
    PrintInts("five_offsets", gp.GetEdgeIndexOffsets());
    const auto res = gp.DijkstraPathsHost(0);
    std::vector<int> prev;
    std::printf("\"five_dist\": [");
    for (size_t i = 0; i < res->size(); ++i) {
        std::printf("%s%.9g", i ? ", " : "", (*res)[i].shortest_distance_);
        prev.push_back((*res)[i].prev_index_);
    }
    std::printf("], ");
    PrintInts("five_prev", prev);
    const auto p04 = gp.DijkstraPath(0, 4);
    PrintInts("five_path", *p04.first);
    const auto p22 = gp.DijkstraPath(2, 2);
    const bool same_node = p22.first->size() == 1 && (*p22.first)[0] == 2 && p22.second == 0.0f;
    const auto dev = gp.DijkstraPaths(0, 3);
    const auto dh = dev->to_host();
    const bool early = dh.size() == 5 && dh[3].shortest_distance_ == 2.0f && std::isinf(dh[4].shortest_distance_) && dh[4].prev_index_ == -1;

    // ---- the zero-weight pair: nodes 1 and 2 joined by weight 0, node 1 entered from node 3
    geometry::Graph<3> trap(std::vector<Eigen::Vector3f>(4, Eigen::Vector3f::Zero()));
    trap.is_directed_ = true;
    trap.AddEdges(std::vector<Eigen::Vector2i>{{1, 2}, {2, 1}, {3, 1}, {3, 0}}, std::vector<float>{0.0f, 0.0f, 1.0f, 4.0f});
    const auto tr = trap.DijkstraPathsHost(3);
    prev.clear();
    for (const auto& r : *tr) prev.push_back(r.prev_index_);
    PrintInts("trap_prev", prev);
    const auto unreachable = trap.DijkstraPath(0, 3);
    const bool no_path = unreachable.first->empty() && std::isinf(unreachable.second);

    // ---- the wall
    const auto roadmap = geometry::Graph<3>::CreateFromAxisAlignedBoundingBox(
            geometry::AxisAlignedBoundingBox3(Eigen::Vector3f(-1.0f, -1.0f, -1.0f), Eigen::Vector3f(1.0f, 1.0f, 1.0f)), Eigen::Vector3i(10, 10, 10));
    const Eigen::Vector3f start(s[0], s[1], s[2]), goal(g[0], g[1], g[2]);
    planning::Pos3DPlanner planner(*roadmap, radius, reach);
    planner.AddObstacle(Wall(ReadRaw<Eigen::Vector3i>(dir + "/wall.i32"), vs));
    const auto path = planner.FindPath(start, goal);
    planner.UpdateGraph();
    const std::vector<float> w = planner.GetGraph().GetEdgeWeights();
    planning::Pos3DPlanner shut(*roadmap, radius, reach);
    shut.AddObstacle(Wall(ReadRaw<Eigen::Vector3i>(dir + "/closed.i32"), vs));
    const auto none = shut.FindPath(start, goal);
    planning::Pos3DPlanner free_space(*roadmap);          // src/tests/planning/planner.cpp
    free_space.AddObstacle(std::make_shared<geometry::PointCloud>());  // (logged as unsupported, not fatal)
    const auto far = free_space.FindPath(Eigen::Vector3f(-1.0f, -0.5f, -0.2f), Eigen::Vector3f(0.8f, 0.9f, 0.7f));
    const bool written = WriteRaw(dir + "/path.f32", path->data(), path->size() * sizeof(Eigen::Vector3f)) &&
                         WriteRaw(dir + "/path_closed.f32", none->data(), none->size() * sizeof(Eigen::Vector3f)) &&
                         WriteRaw(dir + "/path_free.f32", far->data(), far->size() * sizeof(Eigen::Vector3f)) &&
                         WriteRaw(dir + "/weights.f32", w.data(), w.size() * sizeof(float));
    std::printf("\"ctor\": %s, \"same_node\": %s, \"early\": %s, \"no_path\": %s, \"written\": %s, \"nodes\": %zu, \"edges\": %zu}\n",
                ctor ? "true" : "false", same_node ? "true" : "false", early ? "true" : "false", no_path ? "true" : "false",
                written ? "true" : "false", roadmap->points_.size(), roadmap->lines_.size());
    return 0;
}
