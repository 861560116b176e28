// geometry::Image / geometry::RGBDImage through the C++ surface, with the reference's signatures.  argv[1]: a directory
// holding gray.f32 ([23][37] float), color.u8 ([48][64][3] uint8) and depth.u16 ([48][64] uint16); every result goes
// there as <name>.bin with its width, height, channels and bytes per channel in the JSON line this prints.  The directory
// also holds the 5 x 5 inputs of three of the reference's own cases (src/tests/geometry/image.cpp: Filter_Gaussian7,
// CreateFloatImage_3_1_Weighted, ConvertDepthToFloatImage) as ref_f32.u8, ref_rgb.u8 and ref_depth.u8.
// tests/test_gpu_image_cpp.py compiles and runs it and holds the bytes to tests/image_exact.py.
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;
using geometry::Image;
using geometry::RGBDImage;

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

static std::string g_dir, g_json;
static int g_failed = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++g_failed;                                                     \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
        }                                                                   \
    } while (0)

static void Put(const std::string& name, const Image& im) {
    const std::vector<uint8_t> h = im.GetData();
    std::FILE* f = std::fopen((g_dir + "/" + name + ".bin").c_str(), "wb");
    if (!f || (!h.empty() && std::fwrite(h.data(), 1, h.size(), f) != h.size())) ++g_failed;
    if (f) std::fclose(f);
    if (!g_json.empty()) g_json += ", ";
    g_json += "\"" + name + "\": [" + std::to_string(im.width_) + ", " + std::to_string(im.height_) + ", " +
              std::to_string(im.num_of_channels_) + ", " + std::to_string(im.bytes_per_channel_) + "]";
}

static Image Load(const std::string& file, int w, int h, int channels, int bytes) {
    Image im;
    const std::vector<uint8_t> raw = ReadRaw(g_dir + "/" + file);
    EXPECT(raw.size() == (size_t)w * h * channels * bytes);
    im.Prepare(w, h, channels, bytes);
    if (raw.size() == (size_t)w * h * channels * bytes) im.SetData(raw);
    return im;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    g_dir = argv[1];
    const Image gray = Load("gray.f32", 37, 23, 1, 4), color = Load("color.u8", 64, 48, 3, 1), depth = Load("depth.u16", 64, 48, 1, 2);
    EXPECT(!gray.IsEmpty() && gray.BytesPerLine() == 37 * 4 && gray.TestImageBoundary(36.5f, 22.5f) && !gray.TestImageBoundary(36.5f, 22.5f, 1.0f));

    Put("transpose", *gray.Transpose());
    Put("transpose_rgb", *color.Transpose());
    Put("flip_v", *color.FlipVertical());
    Put("flip_h", *depth.FlipHorizontal());
    const std::vector<float> k5 = {0.5f, -1.25f, 2.0f, 0.75f, -0.5f}, k3 = {1.0f, -2.0f, 0.5f};
    Put("horizontal", *gray.FilterHorizontal(k5));
    Put("taps", *gray.Filter(k5, k3));
    Put("gaussian3", *gray.Filter(Image::FilterType::Gaussian3));
    Put("gaussian5", *gray.Filter(Image::FilterType::Gaussian5));
    Put("gaussian7", *gray.Filter(Image::FilterType::Gaussian7));
    Put("sobel_dx", *gray.Filter(Image::FilterType::Sobel3Dx));
    Put("sobel_dy", *gray.Filter(Image::FilterType::Sobel3Dy));
    Put("downsample", *gray.Downsample());
    Put("downsample_rgb", *color.Downsample());
    Put("bilateral", *gray.BilateralFilter(3, 0.5f, 2.0f));
    Put("float_weighted", *color.CreateFloatImage());
    Put("float_equal", *color.CreateFloatImage(Image::ColorToIntensityConversionType::Equal));
    Put("gray_weighted", *color.CreateGrayImage());
    Put("gray_from_float", *gray.CreateGrayImage());
    Put("depth_float", *depth.ConvertDepthToFloatImage());
    Put("depth_float_tum", *depth.ConvertDepthToFloatImage(5000.0f, 4.0f));
    Put("from_float_u8", *gray.CreateImageFromFloatImage<uint8_t>());
    Put("from_float_u16", *depth.CreateFloatImage()->CreateImageFromFloatImage<uint16_t>());
    {
        Image a = gray, b = color;
        EXPECT(&a.ClipIntensity(0.25f, 1.5f) == &a && &b.LinearTransform(1.5f, -40.0f) == &b);
        Put("clip", a);
        Put("linear_u8", b);
        Image c = gray;
        Put("linear_f32", c.LinearTransform(-2.0f, 0.125f));
    }
    const auto pyramid = gray.CreatePyramid(6, true);
    EXPECT(pyramid.size() == 6 && pyramid[5]->IsEmpty() && pyramid[4]->width_ == 2 && pyramid[4]->height_ == 1);
    for (size_t i = 0; i < 5 && i < pyramid.size(); ++i) Put("pyramid" + std::to_string(i), *pyramid[i]);
    const auto plain = gray.CreatePyramid(3, false);
    for (size_t i = 0; i < plain.size(); ++i) Put("plain" + std::to_string(i), *plain[i]);
    const auto sobel = Image::FilterPyramid(plain, Image::FilterType::Sobel3Dx);
    for (size_t i = 0; i < sobel.size(); ++i) Put("plain_sobel" + std::to_string(i), *sobel[i]);
    const auto smooth = Image::BilateralFilterPyramid(plain, 2, 0.5f, 1.5f);
    for (size_t i = 0; i < smooth.size(); ++i) Put("plain_bilateral" + std::to_string(i), *smooth[i]);

    {   // the reference's own 5 x 5 cases, called as its tests call them
        const Image f = Load("ref_f32.u8", 5, 5, 1, 4), rgb = Load("ref_rgb.u8", 5, 5, 3, 1), d = Load("ref_depth.u8", 5, 5, 1, 1);
        Put("ref_gaussian7", *f.CreateFloatImage()->Filter(Image::FilterType::Gaussian7));
        Put("ref_float_3_1", *rgb.CreateFloatImage());
        Put("ref_depth_float", *d.ConvertDepthToFloatImage());
    }

    const auto rgbd = RGBDImage::CreateFromColorAndDepth(color, depth);
    Put("rgbd_color", rgbd->color_);
    Put("rgbd_depth", rgbd->depth_);
    Put("rgbd_raw_color", RGBDImage::CreateFromColorAndDepth(color, depth, 1000.0f, 3.0f, false)->color_);
    Put("redwood_depth", RGBDImage::CreateFromRedwoodFormat(color, depth)->depth_);
    Put("tum_depth", RGBDImage::CreateFromTUMFormat(color, depth)->depth_);
    Put("sun_depth", RGBDImage::CreateFromSUNFormat(color, depth)->depth_);
    Put("nyu_depth", RGBDImage::CreateFromNYUFormat(color, depth)->depth_);
    const auto levels = rgbd->CreatePyramid(3);
    EXPECT(levels.size() == 3);
    for (size_t i = 0; i < levels.size(); ++i) {
        Put("level_color" + std::to_string(i), levels[i]->color_);
        Put("level_depth" + std::to_string(i), levels[i]->depth_);
    }
    const auto gauss = RGBDImage::FilterPyramid(levels, Image::FilterType::Gaussian3);
    for (size_t i = 0; i < gauss.size(); ++i) Put("level_gauss_depth" + std::to_string(i), gauss[i]->depth_);
    const auto bilateral = RGBDImage::BilateralFilterPyramidDepth(levels, 2, 0.1f, 1.5f);
    for (size_t i = 0; i < bilateral.size(); ++i) Put("level_bilateral_depth" + std::to_string(i), bilateral[i]->depth_);

    // what is turned away: logged, an empty image (the object itself for the in-place calls)
    EXPECT(color.Filter(Image::FilterType::Gaussian3)->IsEmpty());
    EXPECT(color.FilterHorizontal(k3)->IsEmpty());
    EXPECT(gray.FilterHorizontal({0.5f, 0.5f})->IsEmpty());
    EXPECT(gray.Filter(std::vector<float>(33, 1.0f), k3)->IsEmpty());
    EXPECT(gray.BilateralFilter(32, 0.5f, 2.0f)->IsEmpty() && gray.BilateralFilter(-1, 0.5f, 2.0f)->IsEmpty());
    EXPECT(color.BilateralFilter(2, 0.5f, 2.0f)->IsEmpty());
    EXPECT(depth.Downsample()->IsEmpty());
    EXPECT(color.CreateImageFromFloatImage<uint8_t>()->IsEmpty());
    EXPECT(depth.CreatePyramid(3).empty());
    EXPECT(RGBDImage::CreateFromColorAndDepth(color, gray)->IsEmpty());
    EXPECT(RGBDImage::CreateFromSUNFormat(color, *depth.CreateFloatImage())->IsEmpty());
    EXPECT(Image().CreateFloatImage()->IsEmpty() && Image().Transpose()->IsEmpty());
    {
        Image b = color;
        EXPECT(&b.ClipIntensity() == &b);
    }

    std::printf("{\"failed\": %d, \"images\": {%s}}\n", g_failed, g_json.c_str());
    return g_failed ? 1 : 0;
}
