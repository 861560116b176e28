// PointCloud::FarthestPointDownSample, GaussianFilter, PassThroughFilter, Crop and RemoveNoneFinitePoints through the
// C++ surface, with the reference's signatures and defaults.  argv[1]: a cloud as raw float32 triples; argv[2]: a
// directory for the outputs (raw float32 triples: fps.f32, gauss.f32, gauss_colors.f32, pass.f32, crop.f32,
// finite.f32).  Prints one JSON line; tests/test_gpu_cloud_filters_cpp.py compiles and runs it and holds the files to
// the C ABI's results.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

static bool Write(const std::string& path, const utility::device_vector<Eigen::Vector3f>& v) {
    const std::vector<Eigen::Vector3f> h = v.to_host();
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite((const void*)h.data(), 3 * sizeof(float), h.size(), f) == h.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / (3 * sizeof(float));
    std::fseek(f, 0, SEEK_SET);
    std::vector<Eigen::Vector3f> pts(n);
    const bool read_ok = std::fread((void*)pts.data(), 3 * sizeof(float), n, f) == n;
    std::fclose(f);
    if (!read_ok) return 2;
    const std::string dir = argv[2];

    geometry::PointCloud pcd;
    pcd.points_ = pts;
    pcd.colors_ = pts;  // (any attribute: it must follow the points)
    const geometry::PointCloud& cpcd = pcd;

    // FarthestPointDownSample(size_t) const
    std::shared_ptr<geometry::PointCloud> fps = cpcd.FarthestPointDownSample(200);
    bool ok = Write(dir + "/fps.f32", fps->points_);
    const size_t fps_none = cpcd.FarthestPointDownSample(0)->points_.size();
    const size_t fps_all = cpcd.FarthestPointDownSample(n)->points_.size();
    const size_t fps_too_many = cpcd.FarthestPointDownSample(n + 1)->points_.size();

    // GaussianFilter(float, float, size_t = 50)
    std::shared_ptr<geometry::PointCloud> gauss = pcd.GaussianFilter(0.05f, 4e-4f);
    ok = ok && Write(dir + "/gauss.f32", gauss->points_) && Write(dir + "/gauss_colors.f32", gauss->colors_);
    const size_t gauss_bad = pcd.GaussianFilter(0.0f, 1.0f)->points_.size() + pcd.GaussianFilter(0.1f, 0.0f)->points_.size() +
                             pcd.GaussianFilter(0.1f, 1.0f, 0)->points_.size() + pcd.GaussianFilter(0.1f, 1.0f, 101)->points_.size();

    // PassThroughFilter(size_t, float, float)
    std::shared_ptr<geometry::PointCloud> pass = pcd.PassThroughFilter(2, 1.0f, 2.0f);
    ok = ok && Write(dir + "/pass.f32", pass->points_);
    const size_t pass_bad_axis = pcd.PassThroughFilter(3, 0.0f, 1.0f)->points_.size();

    // Crop(const AxisAlignedBoundingBox<3>&) const
    const geometry::AxisAlignedBoundingBox<3> box(Eigen::Vector3f(0.5f, 0.5f, 1.0f), Eigen::Vector3f(2.0f, 2.0f, 2.5f));
    std::shared_ptr<geometry::PointCloud> crop = cpcd.Crop(box);
    ok = ok && Write(dir + "/crop.f32", crop->points_);
    const size_t crop_empty_box = cpcd.Crop(geometry::AxisAlignedBoundingBox<3>())->points_.size();
    const size_t crop_own_box = cpcd.Crop(cpcd.GetAxisAlignedBoundingBox())->points_.size();

    // RemoveNoneFinitePoints(bool = true, bool = true): in place, returns *this
    std::vector<Eigen::Vector3f> dirty = pts;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    dirty[1](0) = nan;
    dirty[n / 2](1) = inf;
    dirty[n - 1](2) = -inf;
    geometry::PointCloud d;
    d.points_ = dirty;
    d.colors_ = pts;
    geometry::PointCloud& back = d.RemoveNoneFinitePoints();
    const bool in_place = &back == &d && d.points_.size() == n - 3 && d.colors_.size() == n - 3;
    ok = ok && Write(dir + "/finite.f32", d.colors_);  // (the colours that follow the kept points)
    geometry::PointCloud d2;
    d2.points_ = dirty;
    const size_t nan_only = d2.RemoveNoneFinitePoints(true, false).points_.size();
    const size_t neither = d2.RemoveNoneFinitePoints(false, false).points_.size();

    std::printf("{\"points\": %zu, \"written\": %s, \"fps\": %zu, \"fps_none\": %zu, \"fps_all\": %zu, \"fps_too_many\": %zu, "
                "\"gauss\": %zu, \"gauss_bad\": %zu, \"pass\": %zu, \"pass_bad_axis\": %zu, \"crop\": %zu, "
                "\"crop_empty_box\": %zu, \"crop_own_box\": %zu, \"in_place\": %s, \"nan_only\": %zu, \"neither\": %zu}\n",
                n, ok ? "true" : "false", fps->points_.size(), fps_none, fps_all, fps_too_many, gauss->points_.size(),
                gauss_bad, pass->points_.size(), pass_bad_axis, crop->points_.size(), crop_empty_box, crop_own_box,
                in_place ? "true" : "false", nan_only, neither);
    return 0;
}
