// geometry::keypoint::ComputeISSKeypoints and PointCloud::SelectByMask through the C++ surface.  argv[1]: a cloud as raw
// float32 triples; argv[2]: where the mask goes, one byte per point.  Prints one JSON line;
// tests/test_gpu_iss_keypoints.py compiles and runs it and holds the mask to the C ABI's.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <tuple>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

static std::vector<uint8_t> Bytes(const utility::device_vector<bool>& v) {
    std::vector<uint8_t> h(v.size());
    if (!h.empty()) utility::copy_d2h(h.data(), v.data(), h.size());
    return h;
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

    geometry::PointCloud pcd;
    pcd.points_ = pts;
    pcd.colors_ = pts;  // (any attribute: it must follow the points)
    std::shared_ptr<geometry::PointCloud> kp;
    std::shared_ptr<utility::device_vector<bool>> mask;
    std::tie(kp, mask) = geometry::keypoint::ComputeISSKeypoints(pcd);
    const std::vector<uint8_t> m = Bytes(*mask);
    size_t set = 0;
    for (uint8_t b : m) set += b ? 1 : 0;
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(m.data(), 1, m.size(), f) != m.size()) return 2;
    std::fclose(f);

    // the keypoints are the masked points, in order, with their colours; invert gives the rest
    const std::vector<Eigen::Vector3f> kpts = kp->points_.to_host(), kcol = kp->colors_.to_host();
    bool gathered = kpts.size() == set && kcol.size() == set;
    for (size_t i = 0, j = 0; i < n && gathered; ++i)
        if (m[i]) {
            for (int k = 0; k < 3; ++k) gathered = gathered && kpts[j](k) == pts[i](k) && kcol[j](k) == pts[i](k);
            ++j;
        }
    const size_t rest = pcd.SelectByMask(*mask, true)->points_.size();

    auto again = geometry::keypoint::ComputeISSKeypoints(pcd, 0.0f, 0.0f, 0.975f, 0.975f, 5, 100);
    const bool same = Bytes(*std::get<1>(again)) == m;

    utility::device_vector<bool> wrong(n + 1);
    const size_t wrong_size = pcd.SelectByMask(wrong)->points_.size();
    auto none = geometry::keypoint::ComputeISSKeypoints(geometry::PointCloud());
    const bool empty_ok = std::get<0>(none)->points_.empty() && std::get<1>(none)->empty();
    bool threw = false;
    try {
        geometry::keypoint::ComputeISSKeypoints(pcd, 0.0f, 0.0f, 0.975f, 0.975f, 5, 101);
    } catch (const std::exception&) {
        threw = true;
    }

    std::printf("{\"points\": %zu, \"keypoints\": %zu, \"gathered_in_order\": %s, \"rest\": %zu, \"same_twice\": %s, "
                "\"wrong_size_points\": %zu, \"empty_cloud_empty\": %s, \"max_neighbors_101_throws\": %s}\n",
                n, set, gathered ? "true" : "false", rest, same ? "true" : "false", wrong_size,
                empty_ok ? "true" : "false", threw ? "true" : "false");
    return 0;
}
