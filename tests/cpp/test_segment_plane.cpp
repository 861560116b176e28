// The reference's SegmentPlaneKnownPlane (tests/geometry/pointcloud.cpp:659-674) through the C++ surface, plus the
// argument rules and a slab.  Prints one JSON line; tests/test_gpu_segment_plane.py compiles and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

static bool SamePoints(const std::vector<Eigen::Vector3f>& a, const std::vector<Eigen::Vector3f>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        for (int k = 0; k < 3; ++k)
            if (a[i](k) != b[i](k)) return false;
    return true;
}

int main() {
    const float five[5][3] = {{1, 1, -1}, {2, 2, -5}, {-1, -1, 1}, {-2, -2, 3}, {10, 10, -21}};
    std::vector<Eigen::Vector3f> ref(5);
    for (int i = 0; i < 5; ++i)
        for (int k = 0; k < 3; ++k) ref[i](k) = five[i][k];
    geometry::PointCloud pcd;
    pcd.points_ = ref;

    bool all_seeds = true, select_ok = true, plane_ok = true;
    for (unsigned s = 0; s < 20; ++s) {
        std::srand(s);
        Eigen::Vector4f plane;
        utility::device_vector<size_t> inliers;
        std::tie(plane, inliers) = pcd.SegmentPlane(0.01, 3, 10);
        all_seeds = all_seeds && inliers.size() == 5;
        select_ok = select_ok && SamePoints(pcd.SelectByIndex(inliers)->points_.to_host(), ref);
        // the refit of all five: x = y, its largest-determinant component positive
        plane_ok = plane_ok && std::fabs(std::fabs(plane(0)) - std::sqrt(0.5f)) < 1e-6f && std::fabs(plane(0) + plane(1)) < 1e-6f &&
                   std::fabs(plane(2)) < 1e-6f && std::fabs(plane(3)) < 1e-6f;
    }

    // a slab z ~ 0 with a fifth of clutter; std::srand governs the result
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> uni(-2.0f, 2.0f);
    std::normal_distribution<float> noise(0.0f, 0.004f);
    std::vector<Eigen::Vector3f> pts(20000);
    for (size_t i = 0; i < pts.size(); ++i) {
        pts[i](0) = uni(rng);
        pts[i](1) = uni(rng);
        pts[i](2) = i % 5 == 0 ? uni(rng) : noise(rng);
    }
    geometry::PointCloud slab;
    slab.points_ = pts;
    std::srand(7);
    auto a = slab.SegmentPlane(0.02, 3, 100);
    std::srand(7);
    auto b = slab.SegmentPlane(0.02, 3, 100);
    bool same = std::get<1>(a).size() == std::get<1>(b).size();
    for (int k = 0; k < 4; ++k) same = same && std::get<0>(a)(k) == std::get<0>(b)(k);
    same = same && std::get<1>(a).to_host() == std::get<1>(b).to_host();

    auto two = pcd.SegmentPlane(0.01, 2, 10);
    bool n2_empty = std::get<1>(two).size() == 0;
    for (int k = 0; k < 4; ++k) n2_empty = n2_empty && std::get<0>(two)(k) == 0.0f;
    geometry::PointCloud tiny;
    tiny.points_ = std::vector<Eigen::Vector3f>(ref.begin(), ref.begin() + 2);
    auto few = tiny.SegmentPlane(0.01, 3, 10);
    const bool few_empty = std::get<1>(few).size() == 0 && std::get<0>(few)(0) == 0.0f && std::get<0>(few)(3) == 0.0f;

    std::printf("{\"five_points_all_seeds\": %s, \"select_equals_points\": %s, \"plane_is_x_eq_y\": %s, "
                "\"same_srand_same_result\": %s, \"ransac_n_2_empty\": %s, \"too_few_points_empty\": %s, "
                "\"slab_points\": %zu, \"slab_inliers\": %zu, \"slab_normal_z\": %.7f}\n",
                all_seeds ? "true" : "false", select_ok ? "true" : "false", plane_ok ? "true" : "false",
                same ? "true" : "false", n2_empty ? "true" : "false", few_empty ? "true" : "false", pts.size(),
                std::get<1>(a).size(), std::fabs(std::get<0>(a)(2)));
    return 0;
}
