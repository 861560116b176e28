// collision::ComputeIntersection, Intersection<VoxelGrid> and CreateVoxelGrid through the C++ surface, with the
// reference's signatures: the reference's two unit tests (src/tests/collision/collision.cpp) and one scene per side
// kind.  argv[1]: a directory holding a_keys.i32, b_keys.i32 (raw int32 [m][3]), points.f32, lines.i32, prims.bin (80-byte
// records), cloud.f32, capsule.bin and scene.txt (voxel_size_a, voxel_size_b, origin_a, origin_b, resolution, margin);
// the pairs of every query go there as <name>.i32, the occupancy grid's occupied indices as occ.i32.  Prints one JSON
// line; tests/test_gpu_collision_cpp.py compiles and runs it and holds the files to tests/collision_exact.py.
#include <cstdio>
#include <cstring>
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

static bool WritePairs(const std::string& dir, const char* name, const collision::CollisionResult& r) {
    const std::vector<Eigen::Vector2i> h = r.GetCollisionIndexPairs();
    const std::vector<size_t> first = r.GetFirstCollisionIndices().to_host(), second = r.GetSecondCollisionIndices().to_host();
    bool ok = first.size() == h.size() && second.size() == h.size() && r.IsCollided() == !h.empty();
    for (size_t i = 0; i < h.size() && ok; ++i) ok = (size_t)h[i](0) == first[i] && (size_t)h[i](1) == second[i];
    return ok && WriteRaw(dir + "/" + name + ".i32", h.data(), h.size() * sizeof(Eigen::Vector2i));
}

static geometry::VoxelGrid GridOf(const std::vector<Eigen::Vector3i>& keys, float vs, const Eigen::Vector3f& origin, bool sorted) {
    geometry::VoxelGrid g;
    g.voxel_size_ = vs;
    g.origin_ = origin;
    std::vector<geometry::Voxel> values;
    for (const Eigen::Vector3i& k : keys) values.push_back(geometry::Voxel(k));
    if (sorted) g.AddVoxels(values);  // ascending, known to be
    else g.SetVoxels(keys, values);   // as given
    return g;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    using CT = collision::CollisionResult::CollisionType;

    bool voxel_voxel = false, voxel_lineset = false;
    {  // Collision.VoxelVoxel
        geometry::VoxelGrid voxel1, voxel2;
        const bool none = !collision::ComputeIntersection(voxel1, voxel2)->IsCollided();
        voxel1.voxel_size_ = voxel2.voxel_size_ = 1.0f;
        voxel1.AddVoxel(geometry::Voxel(Eigen::Vector3i(0, 0, 0)));
        voxel2.AddVoxel(geometry::Voxel(Eigen::Vector3i(0, 0, 0)));
        const bool one = collision::ComputeIntersection(voxel1, voxel2)->IsCollided();
        voxel1.AddVoxel(geometry::Voxel(Eigen::Vector3i(5, 0, 0)));
        voxel2.AddVoxel(geometry::Voxel(Eigen::Vector3i(10, 0, 0)));
        const auto res3 = collision::ComputeIntersection(voxel1, voxel2);
        const auto p = res3->GetCollisionIndexPairs();
        voxel_voxel = none && one && p.size() == 1 && p[0](0) == 0 && p[0](1) == 0 && res3->first_ == CT::VoxelGrid;
    }
    {  // Collision.VoxelLineSet
        geometry::VoxelGrid voxel;
        geometry::LineSet<3> lineset;
        const bool none = !collision::ComputeIntersection(voxel, lineset)->IsCollided();
        voxel.voxel_size_ = 1.0f;
        voxel.AddVoxel(geometry::Voxel(Eigen::Vector3i(0, 0, 0)));
        voxel.AddVoxel(geometry::Voxel(Eigen::Vector3i(5, 0, 0)));
        lineset.SetPoints({Eigen::Vector3f(-0.1f, -0.1f, -0.1f), Eigen::Vector3f(-0.1f, -0.1f, 1.1f), Eigen::Vector3f(1.1f, 1.1f, 1.1f)});
        Eigen::Vector2i l0, l1;
        l0(0) = 0, l0(1) = 1, l1(0) = 0, l1(1) = 2;
        lineset.SetLines({l0, l1});
        const auto res2 = collision::ComputeIntersection(voxel, lineset);
        const auto p = res2->GetCollisionIndexPairs();
        voxel_lineset = none && res2->IsCollided() && p.size() == 1 && p[0](0) == 0 && p[0](1) == 1 && res2->second_ == CT::LineSet;
    }

    std::FILE* f = std::fopen((dir + "/scene.txt").c_str(), "r");
    float vs_a = 0, vs_b = 0, margin = 0;
    Eigen::Vector3f oa, ob;
    int res = 0;
    if (!f || std::fscanf(f, "%f %f %f %f %f %f %f %f %d %f", &vs_a, &vs_b, &oa(0), &oa(1), &oa(2), &ob(0), &ob(1), &ob(2), &res, &margin) != 10) return 3;
    std::fclose(f);
    const auto a_keys = ReadRaw<Eigen::Vector3i>(dir + "/a_keys.i32"), b_keys = ReadRaw<Eigen::Vector3i>(dir + "/b_keys.i32");
    const auto points = ReadRaw<Eigen::Vector3f>(dir + "/points.f32"), cloud = ReadRaw<Eigen::Vector3f>(dir + "/cloud.f32");
    const auto lines = ReadRaw<Eigen::Vector2i>(dir + "/lines.i32");
    const collision::PrimitiveArray prims = ReadRaw<collision::PrimitivePack>(dir + "/prims.bin");
    const auto cap = ReadRaw<collision::PrimitivePack>(dir + "/capsule.bin");
    if (a_keys.empty() || b_keys.empty() || points.empty() || lines.empty() || prims.empty() || cloud.empty() || cap.size() != 1) return 4;

    const geometry::VoxelGrid a = GridOf(a_keys, vs_a, oa, true), b = GridOf(b_keys, vs_b, ob, false);
    std::vector<Eigen::Vector3i> reversed(a_keys.rbegin(), a_keys.rend());
    const geometry::VoxelGrid rev = GridOf(reversed, vs_a, oa, false);
    const geometry::LineSet<3> ls(points, lines);
    geometry::OccupancyGrid occ(vs_a, (size_t)res, oa);
    occ.Insert(cloud, oa + Eigen::Vector3f(0.01f, 0.01f, 0.01f));
    const auto occupied = occ.ExtractOccupiedVoxels();
    std::vector<int> occ_index;
    for (const geometry::OccupancyVoxel& v : *occupied)
        for (int k = 0; k < 3; ++k) occ_index.push_back((int)v.grid_index_(k));
    bool written = WriteRaw(dir + "/occ.i32", occ_index.data(), occ_index.size() * sizeof(int));

    written = written && WritePairs(dir, "vv", *collision::ComputeIntersection(a, b, margin));
    written = written && WritePairs(dir, "vl", *collision::ComputeIntersection(a, ls, margin));
    written = written && WritePairs(dir, "lv", *collision::ComputeIntersection(ls, a, margin));
    written = written && WritePairs(dir, "vo", *collision::ComputeIntersection(a, occ, margin));
    written = written && WritePairs(dir, "ov", *collision::ComputeIntersection(occ, a, margin));
    written = written && WritePairs(dir, "ol", *collision::ComputeIntersection(occ, ls, margin));
    written = written && WritePairs(dir, "lo", *collision::ComputeIntersection(ls, occ, margin));
    written = written && WritePairs(dir, "pv", *collision::ComputeIntersection(prims, a, margin));
    written = written && WritePairs(dir, "vp", *collision::ComputeIntersection(a, prims, margin));
    written = written && WritePairs(dir, "po", *collision::ComputeIntersection(prims, occ, margin));
    written = written && WritePairs(dir, "op", *collision::ComputeIntersection(occ, prims, margin));
    // a target kept for several queries: the unsorted grid is sorted once, in the constructor
    const collision::Intersection<geometry::VoxelGrid> kept(rev);
    const bool kept_sorted = kept.sorted_keys_.size() == a_keys.size() && kept.sorted_index_.size() == a_keys.size();
    written = written && WritePairs(dir, "rl", *kept.Compute(ls, margin));
    written = written && WritePairs(dir, "rp", *kept.Compute(prims, margin));
    written = written && WritePairs(dir, "rv", *kept.Compute(b, margin));
    const collision::Intersection<geometry::OccupancyGrid> kept_occ(occ);
    const auto again = kept_occ.Compute(ls, margin);
    const bool same_again = again->GetCollisionIndexPairs().size() == collision::ComputeIntersection(occ, ls, margin)->GetCollisionIndexPairs().size();

    // CreateVoxelGrid, the bounding box, the refusals
    collision::Capsule capsule(cap[0].parameters_(0), cap[0].parameters_(1), cap[0].transform_);
    const auto vg = collision::CreateVoxelGrid(capsule, 0.05f);
    const auto kv = vg->GetVoxels();
    written = written && WriteRaw(dir + "/capsule.i32", kv.first.data(), kv.first.size() * sizeof(Eigen::Vector3i));
    const geometry::AxisAlignedBoundingBox3 box = capsule.GetAxisAlignedBoundingBox();
    const bool refused = collision::CreateVoxelGrid(capsule, 0.0f)->IsEmpty() &&
                         collision::CreateVoxelGrid(collision::Cylinder(0.1f, 0.3f), 0.05f)->IsEmpty() &&
                         !collision::ComputeIntersection(a, b, -1.0f)->IsCollided();
    const auto edges = geometry::LineSet<3>::CreateFromAxisAlignedBoundingBox(box);
    const bool lineset_ok = edges->points_.size() == 8 && edges->lines_.size() == 12 && edges->HasLines() && !edges->HasColors() &&
                            edges->GetMinBound() == box.GetMinBound() && edges->GetMaxBound() == box.GetMaxBound() &&
                            edges->GetLineCoordinate(0).first == box.GetMinBound() && edges->PaintUniformColor(Eigen::Vector3f(1, 0, 0)).HasColors();

    std::printf("{\"voxel_voxel\": %s, \"voxel_lineset\": %s, \"written\": %s, \"kept_sorted\": %s, \"same_again\": %s, \"refused\": %s, "
                "\"lineset\": %s, \"occupied\": %zu, \"capsule\": %zu, \"origin\": [%.9g, %.9g, %.9g], \"box\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g]}\n",
                voxel_voxel ? "true" : "false", voxel_lineset ? "true" : "false", written ? "true" : "false", kept_sorted ? "true" : "false",
                same_again ? "true" : "false", refused ? "true" : "false", lineset_ok ? "true" : "false", occupied->size(), kv.first.size(),
                vg->origin_(0), vg->origin_(1), vg->origin_(2), box.min_bound_(0), box.min_bound_(1), box.min_bound_(2), box.max_bound_(0),
                box.max_bound_(1), box.max_bound_(2));
    return 0;
}
