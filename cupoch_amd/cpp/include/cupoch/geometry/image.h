// cupoch/geometry/image.h -- geometry::Image / geometry::RGBDImage (reference: geometry/image.h,
// geometry/rgbdimage.h): width, height, channels, bytes per channel and the pixel bytes on the device, with the
// reference's image processing -- filters, bilateral filter, pyramids, format conversions, transpose and flips, the
// RGB-D factories -- over the mi_icp_image_* family of include/mi_icp.h, which states what each computes and where it
// departs from the reference.  A format an operation does not take is logged
// ("[<Name>] Unsupported image format.") and the call returns an empty image (the object itself for the two in-place
// calls).  Not provided: FloatValueAt, image file I/O.
#pragma once
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "cupoch/utility/device_vector.h"

namespace cupoch {
namespace geometry {

class Image;
typedef std::vector<std::shared_ptr<Image>> ImagePyramid;

class Image {
public:
    enum class ColorToIntensityConversionType { Equal, Weighted };
    enum class FilterType { Gaussian3, Gaussian5, Gaussian7, Sobel3Dx, Sobel3Dy };

    Image() {}
    Image& Prepare(int width, int height, int num_of_channels, int bytes_per_channel) {
        width_ = width;
        height_ = height;
        num_of_channels_ = num_of_channels;
        bytes_per_channel_ = bytes_per_channel;
        data_.resize((size_t)width * height * num_of_channels * bytes_per_channel);
        return *this;
    }
    Image& Clear() {
        width_ = height_ = num_of_channels_ = bytes_per_channel_ = 0;
        data_.clear();
        return *this;
    }
    void SetData(const std::vector<uint8_t>& bytes) { data_ = bytes; }
    std::vector<uint8_t> GetData() const { return data_.to_host(); }
    bool HasData() const { return width_ > 0 && height_ > 0 && !data_.empty(); }
    bool IsEmpty() const { return !HasData(); }
    int BytesPerLine() const { return width_ * num_of_channels_ * bytes_per_channel_; }
    bool TestImageBoundary(float u, float v, float inner_margin = 0.0f) const {
        return u >= inner_margin && u < width_ - inner_margin && v >= inner_margin && v < height_ - inner_margin;
    }

    std::shared_ptr<Image> ConvertDepthToFloatImage(float depth_scale = 1000.0f, float depth_trunc = 3.0f) const;
    std::shared_ptr<Image> Transpose() const;
    std::shared_ptr<Image> FlipHorizontal() const;
    std::shared_ptr<Image> FlipVertical() const;
    /// `kernel`, `dx`, `dy`: an odd number of taps, at most MI_ICP_IMAGE_MAX_TAPS (host values)
    std::shared_ptr<Image> FilterHorizontal(const std::vector<float>& kernel) const;
    std::shared_ptr<Image> Filter(const std::vector<float>& dx, const std::vector<float>& dy) const;
    std::shared_ptr<Image> Filter(FilterType type) const;
    std::shared_ptr<Image> Downsample() const;
    /// `diameter` is a radius in [0, MI_ICP_IMAGE_MAX_DIAMETER]: the window is (2 diameter + 1)^2
    std::shared_ptr<Image> BilateralFilter(int diameter, float sigma_color, float sigma_space) const;
    Image& ClipIntensity(float min = 0.0f, float max = 1.0f);
    Image& LinearTransform(float scale = 1.0f, float offset = 0.0f);
    std::shared_ptr<Image> CreateGrayImage(ColorToIntensityConversionType type = ColorToIntensityConversionType::Weighted) const;
    std::shared_ptr<Image> CreateFloatImage(ColorToIntensityConversionType type = ColorToIntensityConversionType::Weighted) const;
    /// T: uint8_t (value * 255) or uint16_t (the value); saturating
    template <typename T>
    std::shared_ptr<Image> CreateImageFromFloatImage() const;
    ImagePyramid CreatePyramid(size_t num_of_levels, bool with_gaussian_filter = true) const;
    static ImagePyramid FilterPyramid(const ImagePyramid& input, FilterType type);
    static ImagePyramid BilateralFilterPyramid(const ImagePyramid& input, int diameter, float sigma_color, float sigma_space);

public:
    int width_ = 0;
    int height_ = 0;
    int num_of_channels_ = 0;
    int bytes_per_channel_ = 0;
    utility::device_vector<uint8_t> data_;
};

class RGBDImage;
typedef std::vector<std::shared_ptr<RGBDImage>> RGBDImagePyramid;

class RGBDImage {
public:
    RGBDImage() {}
    RGBDImage(const Image& color, const Image& depth) : color_(color), depth_(depth) {}
    RGBDImage& Clear() {
        color_.Clear();
        depth_.Clear();
        return *this;
    }
    bool IsEmpty() const { return !color_.HasData() || !depth_.HasData(); }

    static std::shared_ptr<RGBDImage> CreateFromColorAndDepth(const Image& color, const Image& depth, float depth_scale = 1000.0f,
                                                              float depth_trunc = 3.0f, bool convert_rgb_to_intensity = true);
    static std::shared_ptr<RGBDImage> CreateFromRedwoodFormat(const Image& color, const Image& depth, bool convert_rgb_to_intensity = true);
    static std::shared_ptr<RGBDImage> CreateFromTUMFormat(const Image& color, const Image& depth, bool convert_rgb_to_intensity = true);
    static std::shared_ptr<RGBDImage> CreateFromSUNFormat(const Image& color, const Image& depth, bool convert_rgb_to_intensity = true);
    static std::shared_ptr<RGBDImage> CreateFromNYUFormat(const Image& color, const Image& depth, bool convert_rgb_to_intensity = true);
    RGBDImagePyramid CreatePyramid(size_t num_of_levels, bool with_gaussian_filter_for_color = true,
                                   bool with_gaussian_filter_for_depth = false) const;
    static RGBDImagePyramid FilterPyramid(const RGBDImagePyramid& rgbd_image_pyramid, Image::FilterType type);
    static RGBDImagePyramid BilateralFilterPyramidDepth(const RGBDImagePyramid& rgbd_image_pyramid, int diameter, float sigma_depth,
                                                        float sigma_space);

public:
    Image color_;
    Image depth_;
};

}  // namespace geometry
}  // namespace cupoch
