// integration::UniformTSDFVolume through the C++ surface, with the reference's signatures: the reference's own
// Constructor test (src/tests/integration/uniform_fsdfvolume.cpp:67-87) and a wall scene.  argv[1]: a depth image
// (raw float32, 64 x 48), argv[2]: its colour image (raw uint8 x 3), argv[3]: a directory for the outputs (raw float32:
// voxels.f32 as [n][5] = tsdf, weight, colour; cloud_{points,normals,colors}.f32; voxel_{points,colors}.f32;
// ray_{points,normals,colors}.f32 of the valid pixels and rayfull_points.f32 of all).  Prints one JSON line;
// tests/test_gpu_tsdf_cpp.py compiles and runs it and holds the files to the restatement of tests/tsdf_exact.py.
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

static std::vector<uint8_t> ReadAll(const char* path) {
    std::vector<uint8_t> out;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return out;
    std::fseek(f, 0, SEEK_END);
    out.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(out.data(), 1, out.size(), f) != out.size()) out.clear();
    std::fclose(f);
    return out;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string dir = argv[3];

    // the reference's Constructor test
    bool ctor = false;
    {
        const float length = 4.0f, sdf_trunc = 0.04f;
        const int resolution = 128;
        integration::UniformTSDFVolume v(length, resolution, sdf_trunc, integration::TSDFVolumeColorType::RGB8);
        ctor = v.voxel_length_ == length / resolution && v.sdf_trunc_ == sdf_trunc &&
               v.color_type_ == integration::TSDFVolumeColorType::RGB8 && v.origin_(0) == 0.0f && v.origin_(1) == 0.0f &&
               v.origin_(2) == 0.0f && v.length_ == length && v.resolution_ == resolution &&
               v.voxel_num_ == resolution * resolution * resolution && (int)v.GetVoxels().size() == v.voxel_num_;
    }

    // the wall scene of tests/test_gpu_tsdf_cpp.py
    const int W = 64, H = 48;
    const std::vector<uint8_t> depth = ReadAll(argv[1]), color = ReadAll(argv[2]);
    if (depth.size() != (size_t)W * H * 4 || color.size() != (size_t)W * H * 3) return 2;
    geometry::Image d, c;
    d.Prepare(W, H, 1, 4).SetData(depth);
    c.Prepare(W, H, 3, 1).SetData(color);
    const geometry::RGBDImage rgbd(c, d);
    const camera::PinholeCameraIntrinsic K(W, H, 60.0f, 60.0f, 31.5f, 23.5f);
    Eigen::Matrix4f E = Eigen::Matrix4f::Identity();
    E(0, 3) = -0.6f;
    E(1, 3) = -0.6f;
    E(2, 3) = 2.0f;  // the camera at (0.6, 0.6, -2), looking along +z

    integration::UniformTSDFVolume vol(1.6f, 32, 0.1f, integration::TSDFVolumeColorType::RGB8, Eigen::Vector3f(0.8f, 0.8f, 0.0f));
    vol.Integrate(rgbd, K, E);
    vol.Integrate(rgbd, K, E);
    // formats the reference turns away: logged, the volume unchanged
    vol.Integrate(geometry::RGBDImage(d, d), K, E);                                        // a float colour image
    vol.Integrate(rgbd, camera::PinholeCameraIntrinsic(32, 24, 30.0f, 30.0f, 15.5f, 11.5f), E);  // sizes differ

    const std::vector<geometry::TSDFVoxel> vox = vol.GetVoxels();
    std::vector<float> flat(vox.size() * 5);
    for (size_t i = 0; i < vox.size(); ++i) {
        flat[i * 5] = vox[i].tsdf_;
        flat[i * 5 + 1] = vox[i].weight_;
        for (int k = 0; k < 3; ++k) flat[i * 5 + 2 + k] = vox[i].color_(k);
    }
    bool ok = WriteRaw(dir + "/voxels.f32", flat.data(), flat.size() * sizeof(float));

    const std::shared_ptr<geometry::PointCloud> cloud = vol.ExtractPointCloud();
    ok = ok && Write(dir + "/cloud_points.f32", cloud->points_) && Write(dir + "/cloud_normals.f32", cloud->normals_) &&
         Write(dir + "/cloud_colors.f32", cloud->colors_);
    const std::shared_ptr<geometry::PointCloud> voxels = vol.ExtractVoxelPointCloud();
    ok = ok && Write(dir + "/voxel_points.f32", voxels->points_) && Write(dir + "/voxel_colors.f32", voxels->colors_);
    const std::shared_ptr<geometry::PointCloud> ray = vol.Raycast(K, E, 0.1f);  // project_valid_depth_only = true
    ok = ok && Write(dir + "/ray_points.f32", ray->points_) && Write(dir + "/ray_normals.f32", ray->normals_) &&
         Write(dir + "/ray_colors.f32", ray->colors_);
    const std::shared_ptr<geometry::PointCloud> full = vol.Raycast(K, E, 0.1f, false);
    ok = ok && Write(dir + "/rayfull_points.f32", full->points_);

    vol.Reset();
    const size_t after_reset = vol.ExtractVoxelPointCloud()->points_.size() + vol.ExtractPointCloud()->points_.size();

    std::printf("{\"constructor\": %s, \"written\": %s, \"cloud\": %zu, \"voxels\": %zu, \"ray\": %zu, \"rayfull\": %zu, "
                "\"has_normals\": %s, \"voxel_cloud_has_normals\": %s, \"after_reset\": %zu}\n",
                ctor ? "true" : "false", ok ? "true" : "false", cloud->points_.size(), voxels->points_.size(),
                ray->points_.size(), full->points_.size(), cloud->HasNormals() ? "true" : "false",
                voxels->HasNormals() ? "true" : "false", after_reset);
    return 0;
}
