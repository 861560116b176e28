// geometry::OccupancyGrid through the C++ surface, with the reference's signatures: the reference's four unit tests
// (src/tests/geometry/occupancygrid.cpp: Bounds, GetVoxel, Insert, SetFreeArea) at the default 512^3, and one scene on a
// grid of 33^3.  argv[1]: the scene's points (raw float32 [n][3]), argv[2]: a text file with 3 floats viewpoint, 3 + 3
// floats free-area corners, 1 float max_range, argv[3]: a directory for the outputs (raw: plane.f32 = the 33^3 log-odds;
// known_index.i32 / known_prob.f32, free_prob.f32, occupied_prob.f32; cloud_points.f32, cloud_colors.f32).  Prints one
// JSON line; tests/test_gpu_occgrid_cpp.py compiles and runs it and holds the files to tests/occgrid_exact.py.
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

static bool WriteRaw(const std::string& path, const void* p, size_t bytes) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

static bool Write(const std::string& path, const utility::device_vector<Eigen::Vector3f>& v) {
    const std::vector<Eigen::Vector3f> h = v.to_host();
    return WriteRaw(path, (const void*)h.data(), h.size() * 3 * sizeof(float));
}

static bool WriteProbs(const std::string& path, const std::vector<geometry::OccupancyVoxel>& v) {
    std::vector<float> p(v.size());
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i].prob_log_;
    return WriteRaw(path, p.data(), p.size() * sizeof(float));
}

static bool Known(const geometry::OccupancyGrid& g, float x, float y, float z) {
    return std::get<0>(g.GetVoxel(Eigen::Vector3f(x, y, z)));
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string dir = argv[3];

    bool bounds = false, get_voxel = false, insert = false, free_area = false;
    {  // Bounds
        geometry::OccupancyGrid g;
        bounds = g.voxel_size_ == 0.05f && g.resolution_ == 512;
        g.origin_ = Eigen::Vector3f(0, 0, 0);
        g.voxel_size_ = 5;
        g.AddVoxel(Eigen::Vector3i(0, 0, 0));
        g.AddVoxel(Eigen::Vector3i(511, 511, 511));
        const Eigen::Vector3f lo = g.GetMinBound(), hi = g.GetMaxBound();
        for (int k = 0; k < 3; ++k) bounds = bounds && lo[k] == -1280.0f && hi[k] == 1280.0f;
        g.AddVoxel(Eigen::Vector3i(512, 0, 0), true);  // outside: logged, nothing changes
        bounds = bounds && g.ExtractKnownVoxels()->size() == 2 && g.GetCenter() == g.origin_;
    }
    {  // GetVoxel
        geometry::OccupancyGrid g;
        g.voxel_size_ = 1.0f;
        const int h = 512 / 2;
        const Eigen::Vector3f at(1.5f, 0.0f, 0.0f);
        g.AddVoxel(Eigen::Vector3i(h + 1, h, h), true);
        const auto r1 = g.GetVoxel(at);
        g.AddVoxel(Eigen::Vector3i(h + 1, h, h), true);
        const auto r2 = g.GetVoxel(at);
        g.AddVoxel(Eigen::Vector3i(h + 1, h, h), false);
        const auto r3 = g.GetVoxel(at);
        get_voxel = std::get<0>(r1) && std::get<1>(r1).prob_log_ == g.prob_hit_log_ && std::get<0>(r2) &&
                    std::get<1>(r2).prob_log_ == g.prob_hit_log_ + g.prob_hit_log_ && std::get<0>(r3) &&
                    std::get<1>(r3).prob_log_ == (g.prob_hit_log_ + g.prob_hit_log_) + g.prob_miss_log_ &&
                    std::get<1>(r3).grid_index_(0) == h + 1 && std::get<1>(r3).color_(2) == 1.0f && g.IsOccupied(at) &&
                    g.IsUnknown(Eigen::Vector3f(2.5f, 0.0f, 0.0f)) && g.IsUnknown(Eigen::Vector3f(1.5f, 256.5f, 0.0f));
    }
    {  // Insert
        geometry::OccupancyGrid g;
        g.origin_ = Eigen::Vector3f(-0.5f, -0.5f, 0.0f);
        g.voxel_size_ = 1.0f;
        thrust::host_vector<Eigen::Vector3f> pts;
        pts.push_back(Eigen::Vector3f(0.0f, 0.0f, 3.5f));
        g.Insert(pts, Eigen::Vector3f::Zero());
        insert = g.ExtractKnownVoxels()->size() == 4 && Known(g, 0, 0, 0.5f) && Known(g, 0, 0, 1.5f) && Known(g, 0, 0, 2.5f) &&
                 Known(g, 0, 0, 3.5f) && !Known(g, 0, 0, 4.5f) && g.ExtractFreeVoxels()->size() == 3 &&
                 g.ExtractOccupiedVoxels()->size() == 1 && geometry::PointCloud::CreateFromOccupancyGrid(g)->points_.size() == 1;
    }
    {  // SetFreeArea
        geometry::OccupancyGrid g;
        g.SetFreeArea(Eigen::Vector3f(0, 0, 0), Eigen::Vector3f(0.1f, 0.1f, 0.1f));
        free_area = g.ExtractFreeVoxels()->size() == 27 && g.ExtractOccupiedVoxels()->size() == 0;
        g.Clear();
        free_area = free_area && g.ExtractKnownVoxels()->size() == 0 && g.resolution_ == 512;
    }

    // the scene of tests/test_gpu_occgrid_cpp.py on a grid of 33^3
    std::vector<float> raw;
    {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        raw.resize((size_t)std::ftell(f) / sizeof(float));
        std::fseek(f, 0, SEEK_SET);
        if (std::fread(raw.data(), sizeof(float), raw.size(), f) != raw.size()) return 2;
        std::fclose(f);
    }
    float a[10];
    {
        std::FILE* f = std::fopen(argv[2], "r");
        if (!f) return 2;
        for (int k = 0; k < 10; ++k)
            if (std::fscanf(f, "%f", &a[k]) != 1) return 2;
        std::fclose(f);
    }
    const size_t n = raw.size() / 3;
    thrust::host_vector<Eigen::Vector3f> host(n);
    for (size_t i = 0; i < n; ++i) host[i] = Eigen::Vector3f(raw[i * 3], raw[i * 3 + 1], raw[i * 3 + 2]);
    const Eigen::Vector3f vp(a[0], a[1], a[2]);

    geometry::OccupancyGrid g(0.1f, 33, Eigen::Vector3f(0.013f, -0.027f, 0.041f));
    g.SetFreeArea(Eigen::Vector3f(a[3], a[4], a[5]), Eigen::Vector3f(a[6], a[7], a[8]));
    const utility::device_vector<Eigen::Vector3f> dev(host);
    g.Insert(dev, vp);                              // device_vector
    g.Insert(host, vp, a[9]);                       // host vector, with a range
    g.Insert(geometry::PointCloud(host), vp);       // PointCloud
    std::vector<Eigen::Vector3i> dup;
    for (int k = 0; k < 40; ++k) dup.push_back(Eigen::Vector3i((k * 7) % 33, (k * 5) % 11, (k * 3) % 33));
    for (int k = 0; k < 40; ++k) dup.push_back(dup[(size_t)((k * 13) % 40)]);
    g.AddVoxels(utility::device_vector<Eigen::Vector3i>(dup), true);
    g.Translate(Eigen::Vector3f(0.05f, 0.0f, -0.05f));
    g.Scale(1.5f);
    g.Insert(dev, vp);

    const std::vector<float> plane = g.GetVoxels();
    bool ok = WriteRaw(dir + "/plane.f32", plane.data(), plane.size() * sizeof(float));
    const auto known = g.ExtractKnownVoxels();
    std::vector<int> idx(known->size() * 3);
    for (size_t i = 0; i < known->size(); ++i)
        for (int k = 0; k < 3; ++k) idx[i * 3 + k] = (int)(*known)[i].grid_index_(k);
    ok = ok && WriteRaw(dir + "/known_index.i32", idx.data(), idx.size() * sizeof(int)) &&
         WriteProbs(dir + "/known_prob.f32", *known) && WriteProbs(dir + "/free_prob.f32", *g.ExtractFreeVoxels()) &&
         WriteProbs(dir + "/occupied_prob.f32", *g.ExtractOccupiedVoxels());
    const std::shared_ptr<geometry::PointCloud> cloud = geometry::PointCloud::CreateFromOccupancyGrid(g);
    ok = ok && Write(dir + "/cloud_points.f32", cloud->points_) && Write(dir + "/cloud_colors.f32", cloud->colors_);
    const Eigen::Vector3f lo = g.GetMinBound(), hi = g.GetMaxBound();

    std::printf("{\"bounds\": %s, \"get_voxel\": %s, \"insert\": %s, \"set_free_area\": %s, \"written\": %s, \"known\": %zu, "
                "\"min_bound\": [%d, %d, %d], \"max_bound\": [%d, %d, %d], \"min\": [%.9g, %.9g, %.9g], "
                "\"max\": [%.9g, %.9g, %.9g], \"cloud\": %zu, \"has_colors\": %s}\n",
                bounds ? "true" : "false", get_voxel ? "true" : "false", insert ? "true" : "false",
                free_area ? "true" : "false", ok ? "true" : "false", known->size(), g.min_bound_[0], g.min_bound_[1],
                g.min_bound_[2], g.max_bound_[0], g.max_bound_[1], g.max_bound_[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2],
                cloud->points_.size(), cloud->HasColors() ? "true" : "false");
    return 0;
}
