// integration::ScalableTSDFVolume through the C++ surface, with the reference's signatures: the constructor's fields
// and a wall scene.  argv[1]: a depth image (raw float32, 64 x 48), argv[2]: its colour image (raw uint8 x 3), argv[3]:
// a directory for the outputs (raw: unit_keys.i32 as [m][3]; units.f32 as [m][4096][5] = tsdf, weight, colour;
// cloud_{points,normals,colors}.f32; voxel_{points,colors}.f32).  Prints one JSON line;
// tests/test_gpu_scalable_tsdf_cpp.py compiles and runs it and holds the files to the restatement of
// tests/scalable_tsdf_exact.py.
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

    // the constructor's fields, the defaults included
    bool ctor = false;
    {
        const float voxel_length = 4.0f / 512.0f, sdf_trunc = 0.04f;
        integration::ScalableTSDFVolume v(voxel_length, sdf_trunc, integration::TSDFVolumeColorType::RGB8);
        integration::ScalableTSDFVolume w(0.02f, 0.06f, integration::TSDFVolumeColorType::NoColor, 2, 7);
        integration::TSDFVolume& base = v;
        ctor = base.voxel_length_ == voxel_length && v.sdf_trunc_ == sdf_trunc &&
               v.color_type_ == integration::TSDFVolumeColorType::RGB8 && v.volume_unit_length_ == voxel_length * 16.0f &&
               v.resolution_ == 16 && v.volume_unit_voxel_num_ == 4096 && v.depth_sampling_stride_ == 4 &&
               w.depth_sampling_stride_ == 2 && v.NumVolumeUnits() == 0 && v.GetVolumeUnits().empty() &&
               v.ExtractPointCloud()->points_.empty();
    }
    bool threw = false;
    try {
        integration::ScalableTSDFVolume bad(0.01f, 0.2f, integration::TSDFVolumeColorType::RGB8);  // sdf_trunc > 16 voxels
    } catch (const std::exception&) {
        threw = true;
    }

    // the wall scene of tests/test_gpu_scalable_tsdf_cpp.py
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

    integration::ScalableTSDFVolume vol(0.05f, 0.1f, integration::TSDFVolumeColorType::RGB8, 2, 8);
    vol.Integrate(rgbd, K, E);
    vol.Integrate(rgbd, K, E);
    // formats the reference turns away: logged, the volume unchanged
    vol.Integrate(geometry::RGBDImage(d, d), K, E);                                        // a float colour image
    vol.Integrate(rgbd, camera::PinholeCameraIntrinsic(32, 24, 30.0f, 30.0f, 15.5f, 11.5f), E);  // sizes differ

    const std::vector<integration::ScalableTSDFVolume::VolumeUnit> units = vol.GetVolumeUnits();
    std::vector<int32_t> keys(units.size() * 3);
    std::vector<float> flat(units.size() * 4096 * 5);
    for (size_t e = 0; e < units.size(); ++e) {
        for (int k = 0; k < 3; ++k) keys[e * 3 + k] = units[e].index_(k);
        for (size_t i = 0; i < 4096; ++i) {
            float* o = &flat[(e * 4096 + i) * 5];
            o[0] = units[e].voxels_[i].tsdf_;
            o[1] = units[e].voxels_[i].weight_;
            for (int k = 0; k < 3; ++k) o[2 + k] = units[e].voxels_[i].color_(k);
        }
    }
    bool ok = WriteRaw(dir + "/unit_keys.i32", keys.data(), keys.size() * sizeof(int32_t)) &&
              WriteRaw(dir + "/units.f32", flat.data(), flat.size() * sizeof(float));

    const std::shared_ptr<geometry::PointCloud> cloud = vol.ExtractPointCloud();
    ok = ok && Write(dir + "/cloud_points.f32", cloud->points_) && Write(dir + "/cloud_normals.f32", cloud->normals_) &&
         Write(dir + "/cloud_colors.f32", cloud->colors_);
    const std::shared_ptr<geometry::PointCloud> voxels = vol.ExtractVoxelPointCloud();
    ok = ok && Write(dir + "/voxel_points.f32", voxels->points_) && Write(dir + "/voxel_colors.f32", voxels->colors_);
    const size_t n_units = vol.NumVolumeUnits();

    vol.Reset();
    const size_t after_reset = vol.ExtractVoxelPointCloud()->points_.size() + vol.ExtractPointCloud()->points_.size() +
                               vol.NumVolumeUnits();

    std::printf("{\"constructor\": %s, \"bad_arguments_throw\": %s, \"written\": %s, \"units\": %zu, \"cloud\": %zu, "
                "\"voxels\": %zu, \"has_normals\": %s, \"voxel_cloud_has_normals\": %s, \"after_reset\": %zu}\n",
                ctor ? "true" : "false", threw ? "true" : "false", ok ? "true" : "false", n_units, cloud->points_.size(),
                voxels->points_.size(), cloud->HasNormals() ? "true" : "false", voxels->HasNormals() ? "true" : "false",
                after_reset);
    return 0;
}
