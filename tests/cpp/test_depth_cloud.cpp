// PointCloud::CreateFromDepthImage and PointCloud::CreateFromRGBDImage through the C++ surface, with the reference's
// signatures.  The 70 x 50 depth and colour images come from integer formulas that tests/test_gpu_depth_cpp.py repeats
// in numpy; the program prints, per cloud, the point count and a 64-bit FNV-1a over the words of each output array
// (little-endian bytes, every NaN replaced by 0x7fc00000) as one JSON line, and the driver holds them to the
// restatement of the contract (tests/depth_exact.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

static uint64_t Fnv(const thrust::host_vector<Eigen::Vector3f>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < v.size(); ++i)
        for (int k = 0; k < 3; ++k) {
            const float f = v[i](k);
            uint32_t w;
            std::memcpy(&w, &f, sizeof(w));
            if (std::isnan(f)) w = 0x7fc00000u;
            for (int b = 0; b < 4; ++b) {
                h ^= (uint64_t)((w >> (8 * b)) & 0xffu);
                h *= 0x100000001b3ull;
            }
        }
    return h;
}

static void Report(const char* name, const geometry::PointCloud& pc, bool last) {
    std::printf("\"%s\": {\"n\": %zu, \"normals\": %zu, \"colors\": %zu, \"h_points\": \"%016llx\", \"h_normals\": \"%016llx\", "
                "\"h_colors\": \"%016llx\"}%s",
                name, pc.points_.size(), pc.normals_.size(), pc.colors_.size(), (unsigned long long)Fnv(pc.GetPoints()),
                (unsigned long long)Fnv(pc.GetNormals()), (unsigned long long)Fnv(pc.GetColors()), last ? "" : ", ");
}

int main() {
    const int W = 70, H = 50;
    std::vector<float> depth((size_t)W * H);
    std::vector<uint8_t> color((size_t)W * H * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int pix = y * W + x;
            float d = (float)(900 + (7 * x + 13 * y) % 700) / 1000.0f;
            if (pix % 11 == 0) d = 0.0f;
            if (pix % 97 == 5) d = std::numeric_limits<float>::infinity();
            if (pix % 89 == 3) d = -1.0f;
            depth[(size_t)pix] = d;
            for (int k = 0; k < 3; ++k) color[(size_t)pix * 3 + k] = (uint8_t)((31 * x + 17 * y + 101 * k) % 256);
        }
    geometry::Image d, c;
    std::vector<uint8_t> raw(depth.size() * sizeof(float));
    std::memcpy(raw.data(), depth.data(), raw.size());
    d.Prepare(W, H, 1, 4).SetData(raw);
    c.Prepare(W, H, 3, 1).SetData(color);
    const camera::PinholeCameraIntrinsic K(W, H, 59.5f, 57.25f, 34.75f, 24.5f);
    Eigen::Matrix4f E = Eigen::Matrix4f::Identity();  // a turn about x (0.6, 0.8: a unit pair in float up to rounding)
    E(1, 1) = 0.8f;
    E(1, 2) = -0.6f;
    E(2, 1) = 0.6f;
    E(2, 2) = 0.8f;
    E(0, 3) = 0.1f;
    E(1, 3) = -0.2f;
    E(2, 3) = 0.3f;

    std::printf("{");
    Report("depth_stride3", *geometry::PointCloud::CreateFromDepthImage(d, K, E, 1000.0f, 1000.0f, 3), false);
    const geometry::RGBDImage rgbd(c, d);
    Report("rgbd_valid", *geometry::PointCloud::CreateFromRGBDImage(rgbd, K, E, true, 1.4f, true), false);
    Report("rgbd_all", *geometry::PointCloud::CreateFromRGBDImage(rgbd, K, E, false, 1.4f, true), true);
    std::printf("}\n");
    return 0;
}
