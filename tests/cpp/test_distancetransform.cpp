// geometry::DistanceTransform through the C++ surface, with the reference's signatures: the reference's unit test
// (src/tests/geometry/distancetransform.cpp: a VoxelGrid of voxel size 1 with the key (5, 5, 5) into a 512^3 transform), a
// scene at 65^3 through the VoxelGrid form, the no-sites case and the two log messages.  argv[1]: the scene's points (raw
// float32 [n][3]), argv[2]: a text file with voxel_size, 3 floats lower bound of the lattice, 3 floats origin of the
// transform, the resolution, argv[3]: a directory for the outputs (raw: keys.i32 = the grid's keys; nearest.i32 [res^3][3]
// with -1 for no site, distance.f32 [res^3]; queried.f32 = GetDistances of the scene's points).  Prints one JSON line;
// tests/test_gpu_edt_cpp.py compiles and runs it and holds the files to tests/edt_exact.py.
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

static bool WritePlane(const std::string& dir, const std::vector<geometry::DistanceVoxel>& v) {
    std::vector<int> idx(v.size() * 3);
    std::vector<float> dist(v.size());
    for (size_t i = 0; i < v.size(); ++i) {
        for (int k = 0; k < 3; ++k) idx[i * 3 + k] = v[i].IsNotSite() ? -1 : (int)v[i].nearest_index_(k);
        dist[i] = v[i].distance_;
    }
    return WriteRaw(dir + "/nearest.i32", idx.data(), idx.size() * sizeof(int)) &&
           WriteRaw(dir + "/distance.f32", dist.data(), dist.size() * sizeof(float));
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string dir = argv[3];

    bool unit = false, defaults = false, no_sites = false, unchanged = false, dense = false;
    {  // the reference's unit test
        geometry::VoxelGrid grid;
        grid.voxel_size_ = 1.0f;
        grid.AddVoxel(geometry::Voxel(Eigen::Vector3i(5, 5, 5)));
        geometry::DistanceTransform dt(1.0f, 512);
        dt.ComputeVoronoiDiagram(grid);
        const auto v = dt.GetVoxel(Eigen::Vector3f(0, 0, 0));
        const geometry::DistanceVoxel& d = std::get<1>(v);
        unit = std::get<0>(v) && !d.IsNotSite() && d.nearest_index_(0) == 261 && d.nearest_index_(1) == 261 &&
               d.nearest_index_(2) == 261 && d.distance_ == std::sqrt(75.0f) && dt.GetDistance(Eigen::Vector3f(5.5f, 5.5f, 5.5f)) == 0.0f &&
               std::isnan(dt.GetDistance(Eigen::Vector3f(256.5f, 0, 0)));
    }
    {  // defaults, the DenseGrid members and the record
        geometry::DistanceTransform dt;
        defaults = dt.voxel_size_ == 0.05f && dt.resolution_ == 512 && dt.origin_ == Eigen::Vector3f(0, 0, 0) && !dt.IsEmpty() &&
                   dt.GetGeometryType() == geometry::Geometry::GeometryType::DistanceTransform;
        const float len = 0.05f * 512.0f * 0.5f;
        defaults = defaults && dt.GetMinBound() == Eigen::Vector3f(-len, -len, -len) && dt.GetMaxBound() == Eigen::Vector3f(len, len, len);
        dt.Translate(Eigen::Vector3f(1, 2, 3)).Scale(2.0f);
        defaults = defaults && dt.GetCenter() == Eigen::Vector3f(1, 2, 3) && dt.voxel_size_ == 0.05f * 2.0f;
        dt.Transform(Eigen::Matrix4f::Identity());  // logged, nothing changes
        dt.Rotate(Eigen::Matrix3f::Identity());
        defaults = defaults && dt.GetCenter() == Eigen::Vector3f(1, 2, 3) && dt.voxel_size_ == 0.05f * 2.0f;
        const geometry::DistanceVoxel v;
        defaults = defaults && v.IsNotSite() && v.distance_ == 0.0f && v.nearest_index_(0) == 0;
    }

    FILE* f = std::fopen(argv[2], "r");
    if (!f) return 2;
    float vs, lo[3], org[3];
    int res;
    if (std::fscanf(f, "%f %f %f %f %f %f %f %d", &vs, &lo[0], &lo[1], &lo[2], &org[0], &org[1], &org[2], &res) != 8) return 2;
    std::fclose(f);
    f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / (3 * sizeof(float));
    std::fseek(f, 0, SEEK_SET);
    std::vector<Eigen::Vector3f> pts(n);
    if (std::fread((void*)pts.data(), 3 * sizeof(float), n, f) != n) return 2;
    std::fclose(f);

    geometry::PointCloud cloud;
    cloud.points_ = pts;
    const Eigen::Vector3f lo3(lo[0], lo[1], lo[2]);
    auto grid = geometry::VoxelGrid::CreateFromPointCloudWithinBounds(cloud, vs, lo3, Eigen::Vector3f(-lo[0], -lo[1], -lo[2]));
    const std::vector<Eigen::Vector3i> keys = grid->voxels_keys_.to_host();
    bool written = WriteRaw(dir + "/keys.i32", (const void*)keys.data(), keys.size() * 3 * sizeof(int));

    geometry::DistanceTransform dt(vs, (size_t)res, Eigen::Vector3f(org[0], org[1], org[2]));
    {  // nothing computed yet: no sites
        const auto v = dt.GetVoxel(dt.origin_);
        no_sites = std::get<0>(v) && std::get<1>(v).IsNotSite() && std::isinf(std::get<1>(v).distance_) &&
                   std::get<1>(v).nearest_index_(0) == 65535 && std::isinf(dt.GetDistance(dt.origin_));
    }
    dt.ComputeEDT(*grid);
    const std::vector<geometry::DistanceVoxel> plane = dt.GetVoxels();
    written = written && WritePlane(dir, plane);
    const std::vector<float> q = dt.GetDistances(cloud.points_)->to_host();
    written = written && WriteRaw(dir + "/queried.f32", q.data(), q.size() * sizeof(float));
    {  // a voxel-size mismatch is logged and changes nothing
        geometry::VoxelGrid other;
        other.voxel_size_ = vs * 2.0f;
        other.AddVoxel(geometry::Voxel(Eigen::Vector3i(0, 0, 0)));
        dt.ComputeEDT(other);
        const std::vector<geometry::DistanceVoxel> again = dt.GetVoxels();
        unchanged = again.size() == plane.size();
        for (size_t i = 0; unchanged && i < plane.size(); ++i)
            unchanged = again[i].distance_ == plane[i].distance_ && again[i].nearest_index_(0) == plane[i].nearest_index_(0) &&
                        again[i].nearest_index_(1) == plane[i].nearest_index_(1) && again[i].nearest_index_(2) == plane[i].nearest_index_(2);
    }
    {  // form 1 with cells on both sides of the border, then Clear
        std::vector<Eigen::Vector3i> cells = {Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(res, 0, 0), Eigen::Vector3i(0, -1, 0)};
        dt.ComputeEDT(utility::device_vector<Eigen::Vector3i>(cells));
        const auto v = dt.GetVoxel(dt.GetMaxBound() - Eigen::Vector3f(vs * 0.5f, vs * 0.5f, vs * 0.5f));
        const float far = std::sqrt((float)(3 * (res - 1) * (res - 1))) * vs;
        dense = std::get<0>(v) && std::get<1>(v).nearest_index_(0) == 0 && std::get<1>(v).distance_ == far;
        dt.Clear();
        dense = dense && std::isinf(dt.GetDistance(dt.origin_));
    }
    std::printf("{\"unit\": %d, \"defaults\": %d, \"no_sites\": %d, \"unchanged\": %d, \"cells\": %d, \"written\": %d, \"keys\": %zu, "
                "\"queries\": %zu}\n",
                (int)unit, (int)defaults, (int)no_sites, (int)unchanged, (int)dense, (int)written, keys.size(), q.size());
    return 0;
}
