// imageproc::SemiGlobalMatching and PointCloud::CreateFromDisparity through the C++ surface, with the reference's
// signatures.  argv[1]: a directory holding left.u8 and right.u8 ([40][130] uint8), want_disp.u8 (the disparity image
// tests/sgm_exact.py computes for them at the defaults), color.u16 ([40][130][3] uint16) and want_points.f32 /
// want_colors.f32 ([40 * 130][3] float) for the intrinsics below.  The program compares on the bytes and also writes
// disp.bin, points.bin and colors.bin there; tests/test_gpu_sgm_cpp.py compiles and runs it and compares them again.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;
using geometry::Image;
using imageproc::SemiGlobalMatching;
using imageproc::SGMOption;

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

// same NaN places, same bits elsewhere
static bool SameWords(const float* a, const std::vector<uint8_t>& want, size_t count) {
    if (want.size() != count * sizeof(float)) return false;
    const float* b = reinterpret_cast<const float*>(want.data());
    for (size_t i = 0; i < count; ++i) {
        if (std::isnan(a[i]) != std::isnan(b[i])) return false;
        if (!std::isnan(a[i]) && std::memcmp(a + i, b + i, sizeof(float)) != 0) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    g_dir = argv[1];
    const int W = 130, H = 40;

    // the option's members, enums and defaults are the reference's (sgm.h:30-70)
    const SGMOption d;
    EXPECT(d.width_ == 0 && d.height_ == 0 && d.p1_ == 10 && d.p2_ == 120 && d.uniqueness_ == 0.95f);
    EXPECT(d.disp_size_ == SGMOption::DisparitySize128 && d.path_type_ == SGMOption::ScanPath8 && d.min_disp_ == 0 && d.lr_max_diff_ == 1);
    EXPECT(SGMOption::DisparitySize64 == 64 && SGMOption::DisparitySize128 == 128 && SGMOption::DisparitySize256 == 256);
    EXPECT(SGMOption::ScanPath4 == 0 && SGMOption::ScanPath8 == 1);
    static_assert(!std::is_copy_constructible<SemiGlobalMatching>::value && !std::is_copy_assignable<SemiGlobalMatching>::value,
                  "SemiGlobalMatching is not copyable");

    const Image left = Load("left.u8", W, H, 1, 1), right = Load("right.u8", W, H, 1, 1);
    SemiGlobalMatching sgm(SGMOption(W, H));
    const auto disp = sgm.ProcessFrame(left, right);
    EXPECT(disp->width_ == W && disp->height_ == H && disp->num_of_channels_ == 1 && disp->bytes_per_channel_ == 1);
    const std::vector<uint8_t> got = disp->GetData();
    EXPECT(got == ReadRaw(g_dir + "/want_disp.u8"));
    Put("disp.bin", got.data(), got.size());
    EXPECT(sgm.ProcessFrame(left, right)->GetData() == got);    // the same object, the same bytes

    // error paths: an empty image, a message, nothing thrown
    SemiGlobalMatching zero{SGMOption()};
    EXPECT(zero.ProcessFrame(left, right)->IsEmpty());
    SemiGlobalMatching bad_p(SGMOption(W, H, 121, 120)), bad_p2(SGMOption(W, H, 10, 225)),
            bad_min(SGMOption(W, H, 10, 120, 0.95f, SGMOption::DisparitySize256, SGMOption::ScanPath8, 1));
    EXPECT(bad_p.ProcessFrame(left, right)->IsEmpty() && bad_p2.ProcessFrame(left, right)->IsEmpty() && bad_min.ProcessFrame(left, right)->IsEmpty());
    const Image color = Load("color.u16", W, H, 3, 2);
    EXPECT(sgm.ProcessFrame(left, color)->IsEmpty());
    Image small;
    small.Prepare(W - 1, H, 1, 1);
    EXPECT(sgm.ProcessFrame(small, small)->IsEmpty());
    SemiGlobalMatching edge(SGMOption(W, H, 0, 224, 0.95f, SGMOption::DisparitySize128, SGMOption::ScanPath4, 128, -1));
    EXPECT(!edge.ProcessFrame(left, right)->IsEmpty());

    // CreateFromDisparity: fx != fy, cx != cx_right
    const camera::PinholeCameraIntrinsic li(W, H, 517.3f, 531.9f, 64.6f, 19.3f), ri(W, H, 517.3f, 531.9f, 61.25f, 19.3f);
    const auto cloud = geometry::PointCloud::CreateFromDisparity(*disp, color, li, ri, 0.0754f);
    const size_t n = (size_t)W * H;
    EXPECT(cloud->points_.size() == n && cloud->colors_.size() == n);
    if (cloud->points_.size() == n && cloud->colors_.size() == n) {
        const auto p = cloud->GetPoints(), c = cloud->GetColors();
        EXPECT(SameWords(p.data()->data(), ReadRaw(g_dir + "/want_points.f32"), n * 3));
        EXPECT(SameWords(c.data()->data(), ReadRaw(g_dir + "/want_colors.f32"), n * 3));
        Put("points.bin", p.data()->data(), n * 3 * sizeof(float));
        Put("colors.bin", c.data()->data(), n * 3 * sizeof(float));
    }
    EXPECT(geometry::PointCloud::CreateFromDisparity(color, color, li, ri, 0.1f)->IsEmpty());
    EXPECT(geometry::PointCloud::CreateFromDisparity(*disp, left, li, ri, 0.1f)->IsEmpty());
    EXPECT(geometry::PointCloud::CreateFromDisparity(*disp, small, li, ri, 0.1f)->IsEmpty());

    std::printf("{\"failed\": %d}\n", g_failed);
    return g_failed ? 1 : 0;
}
