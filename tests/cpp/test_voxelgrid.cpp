// geometry::VoxelGrid through the C++ surface, with the reference's signatures: the reference's three unit tests
// (src/tests/geometry/voxelgrid.cpp: Bounds, GetVoxel, one voxel within bounds) and one scene: two halves of a coloured
// cloud voxelised, merged with +=, carved by a depth map, queried.  argv[1]: points (raw float32 [n][3]), argv[2]:
// colours (the same), argv[3]: a text file with voxel_size, fx fy cx cy, the 16 extrinsic entries row by row, width,
// height, argv[4]: the depth map (raw float32 [height][width]), argv[5]: queries (raw float32 [nq][3]), argv[6]: a
// directory for the outputs (raw: merged_keys.i32 / merged_colors.f32, carved_keys.i32 / carved_colors.f32,
// included.u8, selected_keys.i32).  Prints one JSON line; tests/test_gpu_voxelgrid_cpp.py compiles and runs it and
// holds the files to tests/voxelgrid_exact.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

static std::vector<float> ReadFloats(const char* path) {
    std::vector<float> v;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(float));
    if (!v.empty() && std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) v.clear();
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

static bool WriteGrid(const std::string& dir, const std::string& name, const geometry::VoxelGrid& g) {
    const auto kv = g.GetVoxels();
    std::vector<float> col(kv.second.size() * 3);
    bool same_index = kv.first.size() == kv.second.size();
    for (size_t i = 0; i < kv.second.size(); ++i) {
        for (int d = 0; d < 3; ++d) col[i * 3 + d] = kv.second[i].color_(d);
        same_index = same_index && kv.second[i].grid_index_ == kv.first[i];  // a value carries its key
    }
    return same_index && WriteRaw(dir + "/" + name + "_keys.i32", kv.first.data(), kv.first.size() * 3 * sizeof(int)) &&
           WriteRaw(dir + "/" + name + "_colors.f32", col.data(), col.size() * sizeof(float));
}

static std::vector<Eigen::Vector3f> Rows(const std::vector<float>& v, size_t first, size_t count) {
    std::vector<Eigen::Vector3f> out(count);
    if (count) std::memcpy((void*)out.data(), v.data() + first * 3, count * 3 * sizeof(float));
    return out;
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    const std::string dir = argv[6];

    bool bounds = false, get_voxel = false, one_voxel = false;
    {  // Bounds
        geometry::VoxelGrid g;
        g.origin_ = Eigen::Vector3f(0, 0, 0);
        g.voxel_size_ = 5;
        g.AddVoxel(geometry::Voxel(Eigen::Vector3i(1, 0, 0), Eigen::Vector3f(0, 0, 0)));
        g.AddVoxel(geometry::Voxel(Eigen::Vector3i(0, 2, 0), Eigen::Vector3f(0, 0, 0)));
        g.AddVoxel(geometry::Voxel(Eigen::Vector3i(0, 0, 3), Eigen::Vector3f(0, 0, 0)));
        g.AddVoxel(geometry::Voxel(Eigen::Vector3i(0, 2, 0), Eigen::Vector3f(1, 1, 1)));  // there already: stays as it is
        const Eigen::Vector3f lo = g.GetMinBound(), hi = g.GetMaxBound();
        const auto kv = g.GetVoxels();
        bounds = lo == Eigen::Vector3f(0, 0, 0) && hi == Eigen::Vector3f(10, 15, 20) && kv.first.size() == 3 &&
                 kv.first[0] == Eigen::Vector3i(0, 0, 3) && kv.first[1] == Eigen::Vector3i(0, 2, 0) &&
                 kv.first[2] == Eigen::Vector3i(1, 0, 0) && kv.second[1].color_ == Eigen::Vector3f(0, 0, 0) && g.HasVoxels() &&
                 g.HasColors() && !g.IsEmpty();
        const Eigen::Vector3f c = g.GetVoxelCenterCoordinate(Eigen::Vector3i(0, 2, 0));
        bounds = bounds && c == Eigen::Vector3f(2.5f, 12.5f, 2.5f) && g.GetVoxelCenterCoordinate(Eigen::Vector3i(9, 9, 9)) == Eigen::Vector3f::Zero();
        bounds = bounds && g.GetVoxelBoundingPoints(Eigen::Vector3i(0, 2, 0))[1] == Eigen::Vector3f(0.0f, 10.0f, 5.0f);
        g.Transform(Eigen::Matrix4f::Identity());  // logged, nothing changes
        g.Translate(Eigen::Vector3f(1, 0, 0)).Scale(2.0f);
        bounds = bounds && g.origin_ == Eigen::Vector3f(1, 0, 0) && g.voxel_size_ == 10.0f;
        g.Clear();
        bounds = bounds && g.IsEmpty() && g.voxel_size_ == 0.0f && g.GetMinBound() == g.origin_ && g.GetCenter() == Eigen::Vector3f::Zero();
    }
    {  // GetVoxel
        geometry::VoxelGrid g;
        g.origin_ = Eigen::Vector3f(0, 0, 0);
        g.voxel_size_ = 5;
        const float at[5] = {0.0f, 1.0f, 4.9f, 5.0f, 5.1f};
        const int want[5] = {0, 0, 0, 1, 1};
        get_voxel = true;
        for (int k = 0; k < 5; ++k) get_voxel = get_voxel && g.GetVoxel(Eigen::Vector3f(at[k], at[k], at[k])) == Eigen::Vector3i(want[k], want[k], want[k]);
    }
    {  // one voxel for the point (0.5, 0.5, 0.5) within +-100
        geometry::PointCloud pc;
        pc.points_ = std::vector<Eigen::Vector3f>{Eigen::Vector3f(0.5f, 0.5f, 0.5f)};
        const auto g = geometry::VoxelGrid::CreateFromPointCloudWithinBounds(pc, 1.0f, Eigen::Vector3f(-100, -100, -100),
                                                                             Eigen::Vector3f(100, 100, 100));
        const auto kv = g->GetVoxels();
        one_voxel = kv.first.size() == 1 && kv.first[0] == Eigen::Vector3i(100, 100, 100) && kv.second[0].color_ == Eigen::Vector3f(1, 1, 1);
        const auto bad = geometry::VoxelGrid::CreateFromPointCloudWithinBounds(pc, 0.0f, Eigen::Vector3f(-1, -1, -1), Eigen::Vector3f(1, 1, 1));
        one_voxel = one_voxel && bad->IsEmpty();  // voxel_size <= 0: logged, an empty grid
    }

    // the scene
    const std::vector<float> pts = ReadFloats(argv[1]), col = ReadFloats(argv[2]), depth = ReadFloats(argv[4]), qs = ReadFloats(argv[5]);
    float prm[23] = {0};
    {
        std::FILE* f = std::fopen(argv[3], "r");
        if (!f) return 3;
        for (int k = 0; k < 23; ++k)
            if (std::fscanf(f, "%f", &prm[k]) != 1) return 3;
        std::fclose(f);
    }
    const float vs = prm[0];
    const int width = (int)prm[21], height = (int)prm[22];
    const size_t n = pts.size() / 3, half = n / 2;
    if (n == 0 || col.size() != pts.size() || depth.size() != (size_t)width * height) return 3;
    geometry::PointCloud a, b;
    a.points_ = Rows(pts, 0, half);
    a.colors_ = Rows(col, 0, half);
    b.points_ = Rows(pts, half, n - half);
    b.colors_ = Rows(col, half, n - half);
    const Eigen::Vector3f lo(0, 0, 0), hi(1, 1, 1);
    auto ga = geometry::VoxelGrid::CreateFromPointCloudWithinBounds(a, vs, lo, hi);
    const auto gb = geometry::VoxelGrid::CreateFromPointCloudWithinBounds(b, vs, lo, hi);
    const size_t na = ga->voxels_keys_.size(), nb = gb->voxels_keys_.size();
    *ga += *gb;
    bool written = WriteGrid(dir, "merged", *ga);
    const size_t merged = ga->voxels_keys_.size();
    const Eigen::Vector3f gmin = ga->GetMinBound(), gmax = ga->GetMaxBound(), gc = ga->GetCenter();

    geometry::Image img;
    img.Prepare(width, height, 1, 4);
    img.SetData(std::vector<uint8_t>((const uint8_t*)depth.data(), (const uint8_t*)depth.data() + depth.size() * sizeof(float)));
    camera::PinholeCameraParameters cam;
    cam.intrinsic_.SetIntrinsics(width, height, prm[1], prm[2], prm[3], prm[4]);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) cam.extrinsic_(r, c) = prm[5 + r * 4 + c];
    ga->CarveDepthMap(img, cam, false);
    written = written && WriteGrid(dir, "carved", *ga);
    const size_t carved = ga->voxels_keys_.size();

    const std::vector<bool> inc = ga->CheckIfIncluded(Rows(qs, 0, qs.size() / 3));
    std::vector<uint8_t> inc8(inc.size());
    for (size_t i = 0; i < inc.size(); ++i) inc8[i] = inc[i] ? 1 : 0;
    written = written && WriteRaw(dir + "/included.u8", inc8.data(), inc8.size());

    std::vector<size_t> pick;
    for (size_t i = carved; i-- > 0;)
        if (i % 3 == 0) pick.push_back(i);  // descending: an unsorted grid
    const auto sel = ga->SelectByIndex(utility::device_vector<size_t>(pick), false);
    written = written && WriteGrid(dir, "selected", *sel);
    const std::vector<bool> inc_sel = sel->CheckIfIncluded(Rows(qs, 0, qs.size() / 3));
    size_t agree = 0;
    {
        const auto kept = ga->SelectByIndex(utility::device_vector<size_t>(pick), true);  // the complement
        const std::vector<bool> inc_kept = kept->CheckIfIncluded(Rows(qs, 0, qs.size() / 3));
        for (size_t i = 0; i < inc.size(); ++i) agree += (inc[i] == (inc_sel[i] || inc_kept[i])) && !(inc_sel[i] && inc_kept[i]);
    }
    sel->PaintUniformColor(Eigen::Vector3f(0.5f, 0.25f, 0.125f));
    const auto painted = sel->GetVoxels();
    bool paint = !painted.second.empty();
    for (const geometry::Voxel& v : painted.second) paint = paint && v.color_ == Eigen::Vector3f(0.5f, 0.25f, 0.125f);

    std::printf(
            "{\"bounds\": %s, \"get_voxel\": %s, \"one_voxel\": %s, \"written\": %s, \"paint\": %s, \"na\": %zu, \"nb\": %zu, "
            "\"merged\": %zu, \"carved\": %zu, \"selected\": %zu, \"split_agrees\": %zu, \"min\": [%.9g, %.9g, %.9g], "
            "\"max\": [%.9g, %.9g, %.9g], \"center\": [%.9g, %.9g, %.9g]}\n",
            bounds ? "true" : "false", get_voxel ? "true" : "false", one_voxel ? "true" : "false", written ? "true" : "false",
            paint ? "true" : "false", na, nb, merged, carved, pick.size(), agree, gmin(0), gmin(1), gmin(2), gmax(0), gmax(1),
            gmax(2), gc(0), gc(1), gc(2));
    return 0;
}
