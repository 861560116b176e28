// kinfu::KinfuPipeline through the C++ surface, with the reference's signatures.  argv[1]: a directory holding
// depth_<k>.f32 ([48][64] float, metres) and color_<k>.u8 ([48][64][3] uint8) for k = 0, 1, 2, the frames of
// tests/kinfu_scene.py.  The program runs the pipeline over them with that file's option and writes, row-major, the
// pose after every frame (pose_<k>.bin), and after frame 0 the voxels (tsdf.bin, weight.bin, color.bin) and the model
// pyramid (model_<level>_points.bin / _normals.bin / _colors.bin); tests/test_gpu_kinfu_cpp.py compiles and runs it and
// compares them with the Python mirror's.  Then the refusals, whose lines go to stderr, and Reset.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;
using geometry::Image;
using geometry::RGBDImage;
using kinfu::KinfuOption;
using kinfu::KinfuPipeline;

static std::vector<uint8_t> ReadRaw(const std::string& path) {
    std::vector<uint8_t> v;
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes);
    if (!v.empty() && std::fread((void*)v.data(), 1, v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}

static std::string g_dir;
static int g_failed = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++g_failed;                                                     \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
        }                                                                   \
    } while (0)

static void Put(const std::string& name, const void* data, size_t bytes) {
    std::FILE* f = std::fopen((g_dir + "/" + name).c_str(), "wb");
    if (!f || (bytes && std::fwrite(data, 1, bytes, f) != bytes)) ++g_failed;
    if (f) std::fclose(f);
}

static Image Load(const std::string& file, int w, int h, int channels, int bytes) {
    Image im;
    const std::vector<uint8_t> raw = ReadRaw(g_dir + "/" + file);
    EXPECT(raw.size() == (size_t)w * h * channels * bytes);
    im.Prepare(w, h, channels, bytes);
    if (raw.size() == (size_t)w * h * channels * bytes) im.SetData(raw);
    return im;
}

static void PutVectors(const std::string& name, const std::vector<Eigen::Vector3f>& v) {
    Put(name, v.empty() ? nullptr : v.data()->data(), v.size() * 3 * sizeof(float));
}

static std::vector<float> RowMajor(const Eigen::Matrix4f& T) {
    std::vector<float> out;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out.push_back(T(r, c));
    return out;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    g_dir = argv[1];
    const int W = 64, H = 48, LEVELS = 3, FRAMES = 3;

    // the option's fields and defaults are the reference's (kinfu.h:36-80); the five-argument constructor stays
    const KinfuOption d;
    EXPECT(d.num_pyramid_levels_ == 4 && d.diameter_ == 1 && d.sigma_depth_ == 1.0f && d.sigma_space_ == 10.0f && d.depth_cutoff_ == 3.0f);
    EXPECT(d.tsdf_length_ == 8.0f && d.tsdf_resolution_ == 512 && d.sdf_trunc_ == 0.05f && d.tsdf_origin_ == Eigen::Vector3f::Zero());
    EXPECT(d.tsdf_color_type_ == integration::TSDFVolumeColorType::RGB8 && d.distance_threshold_ == 0.5f);
    EXPECT(d.icp_iterations_ == std::vector<int>({20, 20, 20, 20}) && d.tf_type_ == registration::TransformationEstimationType::PointToPlane);
    static_assert(!std::is_copy_constructible<KinfuPipeline>::value && !std::is_copy_assignable<KinfuPipeline>::value,
                  "KinfuPipeline is not copyable");

    KinfuOption opt(LEVELS, 3.0f, 0.15f, {10, 10, 10});
    opt.tsdf_length_ = 3.0f;
    opt.tsdf_resolution_ = 64;
    opt.sdf_trunc_ = 0.12f;
    opt.tsdf_origin_ = Eigen::Vector3f(-0.75f, -0.75f, 1.2f);
    const camera::PinholeCameraIntrinsic K(W, H, 60.0f, 60.0f, 31.5f, 23.5f);
    KinfuPipeline pipe(K, opt);
    EXPECT(pipe.frame_id_ == 0 && pipe.cur_pose_ == Eigen::Matrix4f::Identity() && pipe.model_pyramid_.empty());
    EXPECT(pipe.intrinsic_.width_ == W && pipe.option_.tsdf_resolution_ == 64 && pipe.volume_.resolution_ == 64);

    std::vector<RGBDImage> frames;
    for (int k = 0; k < FRAMES; ++k)
        frames.emplace_back(Load("color_" + std::to_string(k) + ".u8", W, H, 3, 1), Load("depth_" + std::to_string(k) + ".f32", W, H, 1, 4));
    for (int k = 0; k < FRAMES; ++k) {
        EXPECT(pipe.ProcessFrame(frames[(size_t)k]));
        EXPECT(pipe.frame_id_ == k + 1 && pipe.model_pyramid_.size() == (size_t)LEVELS);
        const std::vector<float> pose = RowMajor(pipe.cur_pose_);
        Put("pose_" + std::to_string(k) + ".bin", pose.data(), pose.size() * sizeof(float));
        if (k > 0) continue;
        EXPECT(pipe.cur_pose_ == Eigen::Matrix4f::Identity());
        const auto voxels = pipe.volume_.GetVoxels();
        std::vector<float> t, w, c;
        for (const auto& v : voxels) {
            t.push_back(v.tsdf_);
            w.push_back(v.weight_);
            for (int j = 0; j < 3; ++j) c.push_back(v.color_(j));
        }
        Put("tsdf.bin", t.data(), t.size() * sizeof(float));
        Put("weight.bin", w.data(), w.size() * sizeof(float));
        Put("color.bin", c.data(), c.size() * sizeof(float));
        for (int i = 0; i < LEVELS && i < (int)pipe.model_pyramid_.size(); ++i) {
            const auto& m = *pipe.model_pyramid_[(size_t)i];
            EXPECT(m.HasPoints() && m.HasNormals() && m.HasColors());
            PutVectors("model_" + std::to_string(i) + "_points.bin", m.GetPoints());
            PutVectors("model_" + std::to_string(i) + "_normals.bin", m.GetNormals());
            PutVectors("model_" + std::to_string(i) + "_colors.bin", m.GetColors());
        }
    }
    EXPECT(!(pipe.cur_pose_ == Eigen::Matrix4f::Identity()));
    EXPECT(pipe.ExtractPointCloud()->HasPoints());

    // refusals: false, a line on stderr, pose, frame count and model as they were
    const Eigen::Matrix4f pose = pipe.cur_pose_;
    const auto model0 = pipe.model_pyramid_[0];
    const auto refused = [&](const RGBDImage& image) {
        EXPECT(!pipe.ProcessFrame(image));
        EXPECT(pipe.cur_pose_ == pose && pipe.frame_id_ == FRAMES && pipe.model_pyramid_.size() == (size_t)LEVELS &&
               pipe.model_pyramid_[0] == model0);
    };
    refused(RGBDImage(Image(), frames[0].depth_));
    pipe.option_.num_pyramid_levels_ = 0;
    refused(frames[0]);
    pipe.option_.num_pyramid_levels_ = 17;
    refused(frames[0]);
    pipe.option_.num_pyramid_levels_ = LEVELS;
    pipe.option_.icp_iterations_ = {10, 10};
    refused(frames[0]);
    pipe.option_.icp_iterations_ = {10, 10, 10};
    Image small_color, small_depth, depth16, gray;
    small_color.Prepare(W / 2, H / 2, 3, 1);
    small_depth.Prepare(W / 2, H / 2, 1, 4);
    refused(RGBDImage(small_color, small_depth));
    depth16.Prepare(W, H, 1, 2);
    depth16.SetData(std::vector<uint8_t>((size_t)W * H * 2, 1));
    refused(RGBDImage(frames[0].color_, depth16));                   // a depth image of uint16: no pyramid of it
    gray.Prepare(W, H, 1, 4);
    gray.SetData(std::vector<uint8_t>((size_t)W * H * 4, 0));
    refused(RGBDImage(gray, frames[0].depth_));                      // float intensity into an RGB8 volume: Integrate's
    EXPECT(pipe.ProcessFrame(frames[2]) && pipe.frame_id_ == FRAMES + 1);

    pipe.Reset();
    EXPECT(pipe.frame_id_ == 0 && pipe.cur_pose_ == Eigen::Matrix4f::Identity() && pipe.model_pyramid_.empty());
    EXPECT(!pipe.volume_.ExtractVoxelPointCloud()->HasPoints());
    EXPECT(pipe.ProcessFrame(frames[0]) && pipe.frame_id_ == 1);

    std::printf("{\"failed\": %d}\n", g_failed);
    return g_failed ? 1 : 0;
}
