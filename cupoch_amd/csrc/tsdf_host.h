// tsdf_host.h -- the host side that mi_tsdf.hip (UniformTSDFVolume) and mi_stsdf.hip (ScalableTSDFVolume) share: the
// checks of an Integrate frame, the cached multiplier image, the filling of TsdfIntegrate and
// the argument checks of the extractions.  The kernels' shared parts are in tsdf_kernels.h.
#pragma once
#include "ctx.h"
#include "tsdf_kernels.h"

namespace mi {
namespace eng {

// an image as the reference's Image describes it
struct TsdfImage {
    const void* data;
    int width, height, channels, bytes_per_channel;
};

// The frame of an Integrate call into a volume of colour type ct: the reference's format checks
// (uniform_tsdfvolume.cu:677-695, scalable_tsdfvolume.cu:318-336; `label` is the class in their message), then the
// sizes and the pointers.  The order is part of the interface.
inline int tsdf_frame_check(mi_icp_ctx* c, const char* label, const char* what, int ct, const TsdfImage& d, const TsdfImage& col,
                            int width, int height, const float* intrinsic4) {
    if (!intrinsic4) return fail(c, MI_ICP_ERR_INVALID, "%s: null intrinsic", what);
    if (d.channels != 1 || d.bytes_per_channel != 4 || d.width != width || d.height != height ||
        (ct == MI_ICP_TSDF_RGB8 && (col.channels != 3 || col.bytes_per_channel != 1)) ||
        (ct == MI_ICP_TSDF_GRAY32 && (col.channels != 1 || col.bytes_per_channel != 4)) ||
        (ct != MI_ICP_TSDF_NO_COLOR && (col.width != width || col.height != height)))
        return fail(c, MI_ICP_ERR_INVALID, "[%s::Integrate] Unsupported image format.", label);
    if (width < 1 || height < 1 || width > MI_ICP_TSDF_MAX_IMAGE_SIDE || height > MI_ICP_TSDF_MAX_IMAGE_SIDE)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad image size (a side is at most %d)", what, MI_ICP_TSDF_MAX_IMAGE_SIDE);
    if (!d.data || (ct != MI_ICP_TSDF_NO_COLOR && !col.data)) return fail(c, MI_ICP_ERR_INVALID, "%s: null image", what);
    return MI_ICP_OK;
}

// the depth -> camera-distance multiplier image of one image size and intrinsic, kept on the volume
struct TsdfMult {
    DevBuf buf;
    int w = 0, h = 0;
    float k[4] = {0, 0, 0, 0};
};

// ... rebuilt when the size or the intrinsic is not the one it was made for
inline int tsdf_mult_ensure(mi_icp_ctx* c, TsdfMult& m, int width, int height, const float* intrinsic4) {
    if (m.buf.p && m.w == width && m.h == height && std::memcmp(m.k, intrinsic4, sizeof(m.k)) == 0) return MI_ICP_OK;
    const int64_t npix = (int64_t)width * height;
    float* out;
    TRY(ensure(c, m.buf, (size_t)npix, &out));
    tsdf_multiplier<<<blocks_for(npix), 256, 0, c->stream>>>(out, width, height, intrinsic4[2], intrinsic4[3], 1.0f / intrinsic4[0],
                                                            1.0f / intrinsic4[1]);
    KCHK(c);
    m.w = width;
    m.h = height;
    std::memcpy(m.k, intrinsic4, sizeof(m.k));
    return MI_ICP_OK;
}

// What tsdf_update_voxel reads of a frame, but for the three image pointers; the span test's fields with it
// (stsdf_integrate does not read those).
inline TsdfIntegrate tsdf_frame_args(const Mat4& E, const float* intrinsic4, int width, int height, float voxel_length,
                                     float sdf_trunc) {
    TsdfIntegrate a = {};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 4; ++k) a.E[r][k] = E.data()[k * 4 + r];
        a.D[r] = voxel_length * a.E[r][2];
    }
    a.fx = intrinsic4[0];
    a.fy = intrinsic4[1];
    a.cx = intrinsic4[2];
    a.cy = intrinsic4[3];
    a.width = width;
    a.height = height;
    a.safe_w = (float)width - 0.0001f;
    a.safe_h = (float)height - 0.0001f;
    a.sdf_trunc = sdf_trunc;
    a.sdf_trunc_inv = (float)(1.0 / (double)sdf_trunc);
    a.cull = (std::fabs(a.cx) <= 65536.0f && std::fabs(a.cy) <= 65536.0f) ? 1 : 0;  // (the sides are at most 2^15)
    a.k_left = a.cx + 1.5f;
    a.k_right = ((float)width + 0.5f) - a.cx;
    a.k_top = a.cy + 1.5f;
    a.k_bottom = ((float)height + 0.5f) - a.cy;
    return a;
}

// an extraction's arguments (no cloud comes in: the sizes are the volume's)
template <class T>
int tsdf_extract_args(mi_icp_ctx* c, const T* t, const std::vector<T*>& list, const char* what, int64_t capacity, int64_t* m,
                      int mem_kind) {
    TRY(check_sizes(c, what, 0, m, mem_kind));
    TRY(handle_check(c, t, list, what, "volume"));
    if (capacity < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative capacity", what);
    return MI_ICP_OK;
}

}  // namespace eng
}  // namespace mi
