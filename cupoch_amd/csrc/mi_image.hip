// mi_image.hip -- geometry::Image / geometry::RGBDImage processing: filters, the pyramid level, the bilateral filter,
// downsampling, format conversions, transpose and flips (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "image_kernels.h"

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// The contract is in include/mi_icp.h ("image"), the kernels in image_kernels.h.  Pixels are device memory; filter taps
// and the spatial table are host arrays that travel with the kernel's arguments, so no call here waits for the stream
// and none uses the context's scratch.

// width and height of an image argument; *empty: nothing to do
static int image_size(mi_icp_ctx* c, const char* what, int width, int height, bool* empty) {
    if (width < 0 || height < 0 || width > MI_ICP_TSDF_MAX_IMAGE_SIDE || height > MI_ICP_TSDF_MAX_IMAGE_SIDE)
        return fail(c, MI_ICP_ERR_INVALID, "%s: width and height must be in [0, %d]", what, MI_ICP_TSDF_MAX_IMAGE_SIDE);
    *empty = width == 0 || height == 0;
    return MI_ICP_OK;
}

static dim3 tiles(int width, int height, int tw, int th) { return dim3((unsigned)((width + tw - 1) / tw), (unsigned)((height + th - 1) / th)); }

static int pixel_format(mi_icp_ctx* c, const char* what, int channels, int bytes, int type, float denom, ImgFormat* f) {
    if (channels < 1 || channels > 4 || bytes < 1 || bytes > 4) return fail(c, MI_ICP_ERR_INVALID, "%s: channels and bytes per channel must be in [1, 4]", what);
    if (type != MI_ICP_IMAGE_EQUAL && type != MI_ICP_IMAGE_WEIGHTED) return fail(c, MI_ICP_ERR_INVALID, "%s: bad conversion type", what);
    f->channels = channels;
    f->bytes = bytes;
    if (type == MI_ICP_IMAGE_EQUAL) {
        f->w0 = f->w1 = f->w2 = (float)(1.0 / 3.0);
    } else {
        f->w0 = 0.2990f;
        f->w1 = 0.5870f;
        f->w2 = 0.1140f;
    }
    f->denom = denom;
    return MI_ICP_OK;
}

static int bilateral(mi_icp_ctx* c, const char* what, const float* src, int width, int height, int diameter, float sigma_color,
                     const float* table, float* dst, int exp_kind) {
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    if (diameter < 0 || diameter > kImgMaxDiameter) return fail(c, MI_ICP_ERR_INVALID, "%s: diameter must be in [0, %d]", what, kImgMaxDiameter);
    if (empty) return MI_ICP_OK;
    if (!src || !dst || !table || src == dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    ImgTable t;
    std::memset(&t, 0, sizeof(t));
    std::memcpy(t.g, table, sizeof(float) * (size_t)(2 * diameter + 1));
    t.d = diameter;
    const int side = kImgBiTile + 2 * diameter;
    const size_t lds = sizeof(float) * (size_t)side * side;
    const dim3 grid = tiles(width, height, kImgBiTile, kImgBiTile);
    if (exp_kind == 1)
        img_bilateral<1><<<grid, kImgThreads, lds, c->stream>>>(src, width, height, t, sigma_color, dst);
    else
        img_bilateral<0><<<grid, kImgThreads, lds, c->stream>>>(src, width, height, t, sigma_color, dst);
    KCHK(c);
    return MI_ICP_OK;
}

extern "C" {

int mi_icp_image_limits(int32_t* max_taps, int32_t* max_diameter) {
    if (max_taps) *max_taps = kImgMaxTaps;
    if (max_diameter) *max_diameter = kImgMaxDiameter;
    return MI_ICP_OK;
}

int mi_icp_image_bilateral_table(int diameter, float sigma_space, float* table) {
    if (diameter < 0 || diameter > kImgMaxDiameter || !table) return MI_ICP_ERR_INVALID;
    const float sigma2 = sigma_space * sigma_space;
    for (int i = 0; i < 2 * diameter + 1; ++i) {
        const float x = (float)(i - diameter);
        const float arg = -(x * x) / (2 * sigma2);
        table[i] = (float)std::exp((double)arg);
    }
    return MI_ICP_OK;
}

int mi_icp_image_filter(mi_icp_ctx* c, const float* src, int width, int height, const float* dx, int nx, const float* dy, int ny,
                        float* dst) {
    const char* what = "image_filter";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    if (!dx || nx < 1 || nx > kImgMaxTaps || nx % 2 != 1) return fail(c, MI_ICP_ERR_INVALID, "%s: dx must have an odd number of taps in [1, %d]", what, kImgMaxTaps);
    if (dy ? (ny < 1 || ny > kImgMaxTaps || ny % 2 != 1) : ny != 0)
        return fail(c, MI_ICP_ERR_INVALID, "%s: dy must have an odd number of taps in [1, %d], or be null with ny 0", what, kImgMaxTaps);
    if (empty) return MI_ICP_OK;
    if (!src || !dst || src == dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    ImgTaps a;
    std::memset(&a, 0, sizeof(a));
    std::memcpy(a.dx, dx, sizeof(float) * (size_t)nx);
    if (dy) std::memcpy(a.dy, dy, sizeof(float) * (size_t)ny);
    a.nx = nx;
    a.ny = ny;
    img_filter<<<tiles(width, height, kImgTileW, kImgTileH), kImgThreads, 0, c->stream>>>(src, width, height, a, dst);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_pyramid_level(mi_icp_ctx* c, const float* src, int width, int height, float* dst) {
    const char* what = "image_pyramid_level";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    if (width / 2 == 0 || height / 2 == 0) return MI_ICP_OK;
    if (!src || !dst || src == dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    img_pyramid_level<<<tiles(width, height, kImgTileW, kImgTileH), kImgThreads, 0, c->stream>>>(src, width, height, dst);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_downsample(mi_icp_ctx* c, const void* src, int width, int height, int channels, int bytes_per_channel, void* dst) {
    const char* what = "image_downsample";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    const bool f32 = channels == 1 && bytes_per_channel == 4, rgb8 = channels == 3 && bytes_per_channel == 1;
    if (!f32 && !rgb8) return fail(c, MI_ICP_ERR_INVALID, "%s: the image must be 1 x float32 or 3 x uint8", what);
    const int hw = width / 2, hh = height / 2;
    const int64_t count = (int64_t)hw * hh;
    if (count == 0) return MI_ICP_OK;
    if (!src || !dst || src == dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    if (f32)
        img_downsample_f32<<<blocks_for(count), 256, 0, c->stream>>>(static_cast<const float*>(src), width, hw, count, static_cast<float*>(dst));
    else
        img_downsample_rgb8<<<blocks_for(count * 3), 256, 0, c->stream>>>(static_cast<const uint8_t*>(src), width, hw, count, static_cast<uint8_t*>(dst));
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_bilateral(mi_icp_ctx* c, const float* src, int width, int height, int diameter, float sigma_color,
                           const float* table, float* dst) {
    return bilateral(c, "image_bilateral", src, width, height, diameter, sigma_color, table, dst, 1);
}

int mi_icp_debug_image_bilateral(mi_icp_ctx* c, const float* src, int width, int height, int diameter, float sigma_color,
                                 const float* table, float* dst, int exp_kind) {
    if (exp_kind != 0 && exp_kind != 1) return c ? fail(c, MI_ICP_ERR_INVALID, "debug_image_bilateral: exp_kind must be 0 or 1") : MI_ICP_ERR_INVALID;
    return bilateral(c, "debug_image_bilateral", src, width, height, diameter, sigma_color, table, dst, exp_kind);
}

int mi_icp_image_create_float(mi_icp_ctx* c, const void* src, int width, int height, int channels, int bytes_per_channel, int type,
                              float* dst) {
    const char* what = "image_create_float";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    ImgFormat f;
    TRY(pixel_format(c, what, channels, bytes_per_channel, type, bytes_per_channel == 1 ? (float)(1.0 / 255.0) : 1.0f, &f));
    if (empty) return MI_ICP_OK;
    if (!src || !dst || src == (const void*)dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    const int64_t count = (int64_t)width * height;
    img_to_float<false><<<blocks_for(count), 256, 0, c->stream>>>(static_cast<const uint8_t*>(src), count, f, 1.0f, 0.0f, dst);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_depth_to_float(mi_icp_ctx* c, const void* src, int width, int height, int channels, int bytes_per_channel,
                                float depth_scale, float depth_trunc, float* dst) {
    const char* what = "image_depth_to_float";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    ImgFormat f;
    TRY(pixel_format(c, what, channels, bytes_per_channel, MI_ICP_IMAGE_WEIGHTED, bytes_per_channel == 1 ? (float)(1.0 / 255.0) : 1.0f, &f));
    if (!(std::fabs(depth_scale) < 2.0e9f) || !(std::fabs(depth_trunc) < 2.0e9f))
        return fail(c, MI_ICP_ERR_INVALID, "%s: depth_scale and depth_trunc must be below 2e9 in size (they are held as int)", what);
    if (empty) return MI_ICP_OK;
    if (!src || !dst || src == (const void*)dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    const int64_t count = (int64_t)width * height;
    img_to_float<true><<<blocks_for(count), 256, 0, c->stream>>>(static_cast<const uint8_t*>(src), count, f, depth_reciprocal((int)depth_scale),
                                                                 (float)(int)depth_trunc, dst);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_create_gray(mi_icp_ctx* c, const void* src, int width, int height, int channels, int bytes_per_channel, int type,
                             uint8_t* dst) {
    const char* what = "image_create_gray";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    const float denom = bytes_per_channel == 1 ? 1.0f : (bytes_per_channel == 2 ? (float)(255.0 / 65535.0) : 255.0f);
    ImgFormat f;
    TRY(pixel_format(c, what, channels, bytes_per_channel, type, denom, &f));
    if (empty) return MI_ICP_OK;
    if (!src || !dst || src == (const void*)dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    const int64_t count = (int64_t)width * height;
    img_to_gray<<<blocks_for(count), 256, 0, c->stream>>>(static_cast<const uint8_t*>(src), count, f, dst);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_from_float(mi_icp_ctx* c, const float* src, int width, int height, int bytes_per_channel, void* dst) {
    const char* what = "image_from_float";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    if (bytes_per_channel != 1 && bytes_per_channel != 2) return fail(c, MI_ICP_ERR_INVALID, "%s: bytes_per_channel must be 1 or 2", what);
    if (empty) return MI_ICP_OK;
    if (!src || !dst || (const void*)src == dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    const int64_t count = (int64_t)width * height;
    if (bytes_per_channel == 1)
        img_from_float<uint8_t><<<blocks_for(count), 256, 0, c->stream>>>(src, count, static_cast<uint8_t*>(dst));
    else
        img_from_float<uint16_t><<<blocks_for(count), 256, 0, c->stream>>>(src, count, static_cast<uint16_t*>(dst));
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_linear_transform(mi_icp_ctx* c, void* data, int width, int height, int channels, int bytes_per_channel, float scale,
                                  float offset) {
    const char* what = "image_linear_transform";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    const bool f32 = channels == 1 && bytes_per_channel == 4, u8 = bytes_per_channel == 1 && channels >= 1 && channels <= 4;
    if (!f32 && !u8) return fail(c, MI_ICP_ERR_INVALID, "%s: the image must be 1 x float32 or uint8", what);
    if (empty) return MI_ICP_OK;
    if (!data) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const int64_t count = (int64_t)width * height * channels;
    if (f32)
        img_linear<float><<<blocks_for(count), 256, 0, c->stream>>>(static_cast<float*>(data), count, scale, offset);
    else
        img_linear<uint8_t><<<blocks_for(count), 256, 0, c->stream>>>(static_cast<uint8_t*>(data), count, scale, offset);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_clip(mi_icp_ctx* c, float* data, int width, int height, float min_value, float max_value) {
    const char* what = "image_clip";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    if (empty) return MI_ICP_OK;
    if (!data) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const int64_t count = (int64_t)width * height;
    img_clip<<<blocks_for(count), 256, 0, c->stream>>>(data, count, min_value, max_value);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_move(mi_icp_ctx* c, const void* src, int width, int height, int bytes_per_pixel, int op, void* dst) {
    const char* what = "image_move";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    if (bytes_per_pixel < 1 || bytes_per_pixel > 16) return fail(c, MI_ICP_ERR_INVALID, "%s: bytes_per_pixel must be in [1, 16]", what);
    if (op != MI_ICP_IMAGE_TRANSPOSE && op != MI_ICP_IMAGE_FLIP_VERTICAL && op != MI_ICP_IMAGE_FLIP_HORIZONTAL)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad op", what);
    if (empty) return MI_ICP_OK;
    if (!src || !dst || src == dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    if (op == MI_ICP_IMAGE_TRANSPOSE) {
        const dim3 grid = tiles(width, height, kImgTrTile, kImgTrTile);
        const bool words = bytes_per_pixel % 4 == 0 && (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 4 == 0;
        if (words) {
            const int upp = bytes_per_pixel / 4;
            img_transpose<uint32_t><<<grid, kImgThreads, (size_t)kImgTrTile * img_tr_stride(upp) * 4, c->stream>>>(
                static_cast<const uint32_t*>(src), width, height, upp, static_cast<uint32_t*>(dst));
        } else {
            img_transpose<uint8_t><<<grid, kImgThreads, (size_t)kImgTrTile * img_tr_stride(bytes_per_pixel), c->stream>>>(
                static_cast<const uint8_t*>(src), width, height, bytes_per_pixel, static_cast<uint8_t*>(dst));
        }
    } else {
        const int64_t bytes = (int64_t)width * height * bytes_per_pixel;
        if (op == MI_ICP_IMAGE_FLIP_VERTICAL)
            img_flip<0><<<blocks_for(bytes), 256, 0, c->stream>>>(static_cast<const uint8_t*>(src), width, height, bytes_per_pixel, static_cast<uint8_t*>(dst));
        else
            img_flip<1><<<blocks_for(bytes), 256, 0, c->stream>>>(static_cast<const uint8_t*>(src), width, height, bytes_per_pixel, static_cast<uint8_t*>(dst));
    }
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_image_depth_format(mi_icp_ctx* c, const uint16_t* src, int width, int height, int format, uint16_t* dst) {
    const char* what = "image_depth_format";
    TRY(check_ctx(c));
    bool empty;
    TRY(image_size(c, what, width, height, &empty));
    if (format != MI_ICP_IMAGE_SUN && format != MI_ICP_IMAGE_NYU) return fail(c, MI_ICP_ERR_INVALID, "%s: bad format", what);
    if (empty) return MI_ICP_OK;
    if (!src || !dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const int64_t count = (int64_t)width * height;
    if (format == MI_ICP_IMAGE_SUN)
        img_depth_format<0><<<blocks_for(count), 256, 0, c->stream>>>(src, count, dst);
    else
        img_depth_format<1><<<blocks_for(count), 256, 0, c->stream>>>(src, count, dst);
    KCHK(c);
    return MI_ICP_OK;
}

}  // extern "C"
