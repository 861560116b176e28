// mi_sgm.hip -- imageproc::SemiGlobalMatching (census, path costs, winner-takes-all, medians, left-right check) and
// PointCloud::CreateFromDisparity (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "sgm_kernels.h"

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// The contract is in include/mi_icp.h ("stereo"), the kernels in sgm_kernels.h.  A matcher belongs to the context that
// made it and is freed with it at the latest.  Its whole workspace is allocated by mi_icp_sgm_create: a frame allocates
// nothing and never waits for the stream.
struct mi_icp_sgm {
    mi_icp_ctx* owner = nullptr;
    int width = 0, height = 0, p1 = 0, p2 = 0, disp_size = 0, npaths = 0, min_disp = 0, lr_max_diff = 0;
    float uniqueness = 0.0f;
    size_t pixels = 0, vol_stride = 0;  // width * height; bytes of one path volume
    uint32_t* census[2] = {nullptr, nullptr};
    uint8_t* vol = nullptr;     // npaths path volumes [y][x][d], one byte a cost
    uint16_t* lmap = nullptr;   // the left map before its median
    uint32_t* rcand = nullptr;  // the right map before its median, as (S << 8 | d) or kSgmNoCandidate
    bool has_frame = false;
    void free_buffers() {
        for (int k = 0; k < 2; ++k)
            if (census[k]) (void)hipFree(census[k]);
        if (vol) (void)hipFree(vol);
        if (lmap) (void)hipFree(lmap);
        if (rcand) (void)hipFree(rcand);
    }
};

void mi::eng::sgm_release_all(mi_icp_ctx* c) { handle_release_all(c->sgm_matchers); }

static int sgm_check(mi_icp_ctx* c, const mi_icp_sgm* s, const char* what) {
    return handle_check(c, s, c->sgm_matchers, what, "matcher");
}

static dim3 pixel_grid(int width, int height, int planes = 1) {
    return dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4), (unsigned)planes);
}

static int census_size(mi_icp_ctx* c, const char* what, int width, int height) {
    if (width < 1 || height < 1 || width > MI_ICP_SGM_MAX_SIDE || height > MI_ICP_SGM_MAX_SIDE)
        return fail(c, MI_ICP_ERR_INVALID, "%s: width and height must be in [1, %d]", what, MI_ICP_SGM_MAX_SIDE);
    return MI_ICP_OK;
}

template <int DPL>
static void launch_frame(mi_icp_ctx* c, const mi_icp_sgm* s) {
    const int W = s->width, H = s->height;
    const int lines = std::max(W, H);
    sgm_paths<DPL><<<dim3((unsigned)((lines + 3) / 4), (unsigned)s->npaths), 256, 0, c->stream>>>(s->census[0], s->census[1], W, H, s->min_disp,
                                                                                                 s->p1, s->p2, s->vol, s->vol_stride);
    const dim3 tiles((unsigned)((W + kSgmTile - 1) / kSgmTile), (unsigned)H);
    if (s->npaths == 8)
        sgm_wta<DPL, 8><<<tiles, 256, 0, c->stream>>>(s->vol, s->vol_stride, W, s->min_disp, s->uniqueness, s->lmap, s->rcand);
    else
        sgm_wta<DPL, 4><<<tiles, 256, 0, c->stream>>>(s->vol, s->vol_stride, W, s->min_disp, s->uniqueness, s->lmap, s->rcand);
}

extern "C" {

int mi_icp_sgm_limits(int32_t* max_side, int32_t* max_p2) {
    if (max_side) *max_side = MI_ICP_SGM_MAX_SIDE;
    if (max_p2) *max_p2 = MI_ICP_SGM_MAX_P2;
    return MI_ICP_OK;
}

int mi_icp_sgm_create(mi_icp_ctx* c, int width, int height, int p1, int p2, float uniqueness, int disp_size, int path_type,
                      int min_disp, int lr_max_diff, mi_icp_sgm** out) {
    const char* what = "sgm_create";
    TRY(check_ctx(c));
    if (!out) return fail(c, MI_ICP_ERR_INVALID, "%s: out is null", what);
    *out = nullptr;
    TRY(census_size(c, what, width, height));
    if (p1 < 0 || p1 > p2 || p2 > MI_ICP_SGM_MAX_P2) return fail(c, MI_ICP_ERR_INVALID, "%s: 0 <= p1 <= p2 <= %d does not hold", what, MI_ICP_SGM_MAX_P2);
    if (disp_size != 64 && disp_size != 128 && disp_size != 256) return fail(c, MI_ICP_ERR_INVALID, "%s: disp_size must be 64, 128 or 256", what);
    if (path_type != MI_ICP_SGM_PATH4 && path_type != MI_ICP_SGM_PATH8) return fail(c, MI_ICP_ERR_INVALID, "%s: bad path_type", what);
    if (min_disp < 0 || min_disp + disp_size > 256) return fail(c, MI_ICP_ERR_INVALID, "%s: min_disp >= 0 and min_disp + disp_size <= 256 do not hold", what);
    mi_icp_sgm* s = new mi_icp_sgm;
    s->owner = c;
    s->width = width;
    s->height = height;
    s->p1 = p1;
    s->p2 = p2;
    s->uniqueness = uniqueness;
    s->disp_size = disp_size;
    s->npaths = path_type == MI_ICP_SGM_PATH8 ? 8 : 4;
    s->min_disp = min_disp;
    s->lr_max_diff = lr_max_diff;
    s->pixels = (size_t)width * height;
    s->vol_stride = s->pixels * (size_t)disp_size;
    const size_t total = s->vol_stride * s->npaths;
    if (hipMalloc((void**)&s->census[0], s->pixels * 4) != hipSuccess || hipMalloc((void**)&s->census[1], s->pixels * 4) != hipSuccess ||
        hipMalloc((void**)&s->vol, total) != hipSuccess || hipMalloc((void**)&s->lmap, s->pixels * 2) != hipSuccess ||
        hipMalloc((void**)&s->rcand, s->pixels * 4) != hipSuccess) {
        (void)hipGetLastError();
        s->free_buffers();
        delete s;
        return fail(c, MI_ICP_ERR_HIP, "%s: out of memory for the workspace (%zu bytes of path costs)", what, total);
    }
    c->sgm_matchers.push_back(s);
    *out = s;
    return MI_ICP_OK;
}

int mi_icp_sgm_destroy(mi_icp_ctx* c, mi_icp_sgm* s) {
    return handle_destroy(c, s, c->sgm_matchers, "sgm_destroy", "matcher");
}

int mi_icp_sgm_census(mi_icp_ctx* c, const uint8_t* src, int width, int height, uint32_t* dst) {
    const char* what = "sgm_census";
    TRY(check_ctx(c));
    TRY(census_size(c, what, width, height));
    if (!src || !dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    sgm_census<<<pixel_grid(width, height), 256, 0, c->stream>>>(src, src, width, height, dst, dst);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_sgm_process(mi_icp_ctx* c, mi_icp_sgm* s, const uint8_t* left, const uint8_t* right, uint8_t* dst) {
    const char* what = "sgm_process";
    TRY(check_ctx(c));
    TRY(sgm_check(c, s, what));
    if (!left || !right || !dst || dst == left || dst == right) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    const int W = s->width, H = s->height;
    sgm_census<<<pixel_grid(W, H, 2), 256, 0, c->stream>>>(left, right, W, H, s->census[0], s->census[1]);
    KCHK(c);
    HIPCHK(c, hipMemsetAsync(s->rcand, 0xff, s->pixels * 4, c->stream));
    if (s->disp_size == 64)
        launch_frame<1>(c, s);
    else if (s->disp_size == 128)
        launch_frame<2>(c, s);
    else
        launch_frame<4>(c, s);
    KCHK(c);
    sgm_tail<<<pixel_grid(W, H), 256, 0, c->stream>>>(s->lmap, s->rcand, W, H, s->min_disp, s->lr_max_diff, dst);
    KCHK(c);
    s->has_frame = true;
    return MI_ICP_OK;
}

int mi_icp_sgm_get_sums(mi_icp_ctx* c, mi_icp_sgm* s, uint16_t* dst) {
    const char* what = "sgm_get_sums";
    TRY(check_ctx(c));
    TRY(sgm_check(c, s, what));
    if (!s->has_frame) return fail(c, MI_ICP_ERR_STATE, "%s: no frame has been processed", what);
    if (!dst) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    sgm_sums<<<(unsigned)((s->vol_stride + 255) / 256), 256, 0, c->stream>>>(s->vol, s->vol_stride, s->npaths, s->vol_stride, dst);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_create_from_disparity(mi_icp_ctx* c, const uint8_t* disp, const void* color, int width, int height, int bytes_per_channel,
                                 const float* q, float* points, float* colors) {
    const char* what = "create_from_disparity";
    TRY(check_ctx(c));
    if (width < 0 || height < 0 || width > MI_ICP_TSDF_MAX_IMAGE_SIDE || height > MI_ICP_TSDF_MAX_IMAGE_SIDE)
        return fail(c, MI_ICP_ERR_INVALID, "%s: width and height must be in [0, %d]", what, MI_ICP_TSDF_MAX_IMAGE_SIDE);
    if (bytes_per_channel != 1 && bytes_per_channel != 2) return fail(c, MI_ICP_ERR_INVALID, "%s: bytes_per_channel must be 1 or 2", what);
    if (!q) return fail(c, MI_ICP_ERR_INVALID, "%s: q is null", what);
    const int64_t count = (int64_t)width * height;
    if (count == 0) return MI_ICP_OK;
    if (!disp || !color || !points || !colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const DisparityQ dq = {q[0], q[1], q[2], q[3], q[4], q[5], q[6]};
    if (bytes_per_channel == 1)
        disparity_points<uint8_t><<<blocks_for(count), 256, 0, c->stream>>>(disp, static_cast<const uint8_t*>(color), width, count, dq, 255.0f, points, colors);
    else
        disparity_points<uint16_t><<<blocks_for(count), 256, 0, c->stream>>>(disp, static_cast<const uint16_t*>(color), width, count, dq, 65535.0f, points, colors);
    KCHK(c);
    return MI_ICP_OK;
}

}  // extern "C"
