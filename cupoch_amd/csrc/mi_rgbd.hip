// mi_rgbd.hip -- depth / RGB-D frame -> cloud (PointCloud::CreateFromDepthImage / CreateFromRGBDImage) and RGB-D odometry
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "depth_kernels.h"
#include "odometry.h"

using namespace mi;
using namespace mi::eng;
using host::Mat4;

namespace mi {
namespace eng {
// column-major general inverse, in double (the camera pose of an extrinsic)
bool invert4(const float* M, float* out) {
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) {
            a[r][k] = (double)M[k * 4 + r];
            a[r][4 + k] = (r == k) ? 1.0 : 0.0;
        }
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (!(std::fabs(a[piv][col]) > 0.0)) return false;
        if (piv != col)
            for (int k = 0; k < 8; ++k) std::swap(a[piv][k], a[col][k]);
        const double d = a[col][col];
        for (int k = 0; k < 8; ++k) a[col][k] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
            if (f != 0.0)
                for (int k = 0; k < 8; ++k) a[r][k] -= f * a[col][k];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) out[k * 4 + r] = (float)a[r][4 + k];
    return true;
}
}  // namespace eng
}  // namespace mi

extern "C" {

// ---------------------------------------------------------------------------
// PointCloud::CreateFromDepthImage / CreateFromRGBDImage (geometry/pointcloud_factory.cu)
int mi_icp_create_from_depth(mi_icp_ctx* c, const void* depth, int depth_type, const void* color, int color_type,
                             int width, int height, const float* intrinsic4, const float* extrinsic,
                             float depth_scale, float depth_trunc, float depth_cutoff, int stride, int rgbd,
                             int compute_normals, int valid_only, float* out_xyz, float* out_normals,
                             float* out_colors, int64_t* m, int mem_kind) {
    TRY(check_sizes(c, "create_from_depth", 0, m, mem_kind));  // (the image's sizes are looked at below, with their own message)
    if (width < 0 || height < 0 || stride < 1 || !intrinsic4 || (depth_type != MI_ICP_DEPTH_F32 && depth_type != MI_ICP_DEPTH_U16) ||
        (color_type != MI_ICP_COLOR_NONE && color_type != MI_ICP_COLOR_U8X3 && color_type != MI_ICP_COLOR_F32X1))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: bad arguments");
    if (rgbd && (stride != 1 || depth_type != MI_ICP_DEPTH_F32))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: an RGB-D image has a float depth and stride 1");
    if (!rgbd && (color || compute_normals || !valid_only))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: colours, normals and valid_only = 0 belong to the RGB-D form");
    if ((color != nullptr) != (color_type != MI_ICP_COLOR_NONE))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: color and color_type disagree");
    const int64_t npix = (int64_t)width * height;
    const int64_t count = (int64_t)(width / stride) * (height / stride);
    if (npix > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: image too large");
    if (count == 0) return MI_ICP_OK;
    if (!depth || !out_xyz || (color && !out_colors) || (compute_normals && !out_normals))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: null buffer");

    DepthArgs a;
    const size_t dbytes = (size_t)npix * (depth_type == MI_ICP_DEPTH_U16 ? 2 : 4);
    const size_t cbytes = color ? (size_t)npix * (color_type == MI_ICP_COLOR_U8X3 ? 3 : 4) : 0;
    const uint8_t *dd, *dc;
    TRY(to_device(c, (const uint8_t*)depth, dbytes, mem_kind, c->stage[0], &dd));
    TRY(to_device(c, (const uint8_t*)color, cbytes, mem_kind, c->stage[1], &dc));
    a.depth = dd;
    a.color = dc;
    a.width = width;
    a.height = height;
    a.stride = stride;
    a.depth_u16 = depth_type == MI_ICP_DEPTH_U16;
    a.color_kind = color_type;
    a.rgbd = rgbd ? 1 : 0;
    a.depth_recip = depth_reciprocal((int)depth_scale);  // image.cu:340-343 holds both as int
    a.depth_trunc = (int)depth_trunc;
    a.depth_cutoff = depth_cutoff;
    a.fx = intrinsic4[0];
    a.fy = intrinsic4[1];
    a.cx = intrinsic4[2];
    a.cy = intrinsic4[3];
    const Mat4 E = load_T(extrinsic);
    if (!invert4(E.data(), a.pose)) return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: singular extrinsic");

    const int nb = blocks_for(count);
    uint32_t* pos = nullptr;
    int64_t kept = count;
    if (valid_only) {  // the flags become their own positions
        const uint32_t* total;
        TRY(ensure(c, c->flags, (size_t)count, &pos));
        depth_valid_flags<<<nb, 256, 0, c->stream>>>(a, count, pos);
        KCHK(c);
        TRY(scan_into(c, pos, pos, count, &total));
        TRY(read_total(c, total));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        kept = (int64_t)c->u_host[0];
    }
    float* const out[3] = {out_xyz, compute_normals ? out_normals : nullptr, color ? out_colors : nullptr};
    TRY(cloud_emit(c, out, out, count, kept, mem_kind, c->stage + 3, [&](float* const dst[3]) {
        depth_emit<<<nb, 256, 0, c->stream>>>(a, count, pos, dst[0], dst[1], dst[2]);
    }));
    *m = kept;
    return MI_ICP_OK;
}

// ---------------------------------------------------------------------------
// odometry::ComputeRGBDOdometry (odometry/odometry.cu); helpers above the extern "C" block
static int rgbd_odometry_impl(mi_icp_ctx* c, const float* source_color, const float* source_depth,
                              const float* target_color, const float* target_depth, int width, int height,
                              const float* intrinsic4, const float* odo_init, int jacobian,
                              const mi_icp_odometry_option* option, int* success, float* transformation16,
                              double* information36, int mem_kind, bool weighted, const float* prev_twist6,
                              float* twist6) {
    TRY(check_ctx(c, mem_kind, "compute_rgbd_odometry"));
    c->od_levels = 0;  // (mi_icp_debug_odometry_image: nothing to show until this call has run)
    if (twist6)
        for (int i = 0; i < 6; ++i) twist6[i] = 0.0f;
    if (!success || !transformation16 || !information36 || !intrinsic4 || !option)
        return fail(c, MI_ICP_ERR_INVALID, "compute_rgbd_odometry: null argument");
    *success = 0;
    const Mat4 I4 = host::identity4();
    std::memcpy(transformation16, I4.data(), 16 * sizeof(float));
    for (int i = 0; i < 36; ++i) information36[i] = (i % 7 == 0) ? 1.0 : 0.0;
    if (width <= 0 || height <= 0 || (int64_t)width * height > 0x3fffffffll || !source_color || !source_depth ||
        !target_color || !target_depth)
        return fail(c, MI_ICP_ERR_INVALID, "compute_rgbd_odometry: bad image arguments");
    if (jacobian != MI_ICP_ODOMETRY_COLOR_TERM && jacobian != MI_ICP_ODOMETRY_HYBRID_TERM)
        return fail(c, MI_ICP_ERR_INVALID, "compute_rgbd_odometry: unknown jacobian type %d", jacobian);
    const int L = option->num_levels;
    if (L < 1 || L > MI_ICP_ODOMETRY_MAX_LEVELS || (width >> (L - 1)) < 1 || (height >> (L - 1)) < 1)
        return fail(c, MI_ICP_ERR_INVALID, "compute_rgbd_odometry: bad number of pyramid levels");

    const int64_t n0 = (int64_t)width * height;
    const float *in_sc, *in_sd, *in_tc, *in_td;
    TRY(to_device(c, source_color, (size_t)n0, mem_kind, c->stage[0], &in_sc));
    TRY(to_device(c, source_depth, (size_t)n0, mem_kind, c->stage[1], &in_sd));
    TRY(to_device(c, target_color, (size_t)n0, mem_kind, c->stage[2], &in_tc));
    TRY(to_device(c, target_depth, (size_t)n0, mem_kind, c->stage[3], &in_td));

    // one arena: per level colour + depth of both frames, a scratch image, and (target) 4 gradient images
    int lw[MI_ICP_ODOMETRY_MAX_LEVELS], lh[MI_ICP_ODOMETRY_MAX_LEVELS];
    size_t total = 0;
    for (int l = 0; l < L; ++l) {
        lw[l] = l ? lw[l - 1] / 2 : width;
        lh[l] = l ? lh[l - 1] / 2 : height;
        total += (size_t)lw[l] * lh[l] * 8;
    }
    total += (size_t)n0 + 64;
    float* arena;
    TRY(ensure(c, c->stage[4], total, &arena));
    double *sums, *rows;  // the 32 totals; the rows of od_accumulate's larger grids (the ICP reduction's row buffer: transient there too)
    TRY(ensure(c, c->sys_dev, kSysSize, &sums));
    TRY(ensure(c, c->partial, (size_t)kSysSize * kOdMaxBlocks, &rows));
    float *col[2][MI_ICP_ODOMETRY_MAX_LEVELS], *dep[2][MI_ICP_ODOMETRY_MAX_LEVELS], *grad[4][MI_ICP_ODOMETRY_MAX_LEVELS];
    {
        float* p = arena;
        for (int l = 0; l < L; ++l) {
            const size_t n = (size_t)lw[l] * lh[l];
            for (int s = 0; s < 2; ++s) {
                col[s][l] = p;
                p += n;
                dep[s][l] = p;
                p += n;
            }
            for (int g = 0; g < 4; ++g) {
                grad[g][l] = p;
                p += n;
            }
        }
    }
    float* scratch = arena + (total - (size_t)n0 - 64);
    auto blocks = [](int64_t n) { return (int)((n + kOdThreads - 1) / kOdThreads); };

    // ---- InitializeRGBDOdometry (odometry.cu:498-528)
    for (int s = 0; s < 2; ++s) {
        od_filter3<0, false><<<blocks(n0), kOdThreads, 0, c->stream>>>(s ? in_tc : in_sc, width, height, col[s][0], 0.0f, 0.0f);
        od_filter3<0, true><<<blocks(n0), kOdThreads, 0, c->stream>>>(s ? in_td : in_sd, width, height, dep[s][0],
                                                                       option->min_depth, option->max_depth);
    }
    KCHK(c);
    OdCamera cam[MI_ICP_ODOMETRY_MAX_LEVELS];
    {
        const float k0[9] = {intrinsic4[0], 0.0f, intrinsic4[2], 0.0f, intrinsic4[1], intrinsic4[3], 0.0f, 0.0f, 1.0f};
        std::memcpy(cam[0].k, k0, sizeof(k0));
        for (int l = 1; l < L; ++l) {  // CreateCameraMatrixPyramid (:332-347)
            for (int i = 0; i < 9; ++i) cam[l].k[i] = (float)(0.5 * (double)cam[l - 1].k[i]);
            cam[l].k[8] = 1.0f;
        }
    }
    // the running transformation and everything derived from it live on the device (OdState);
    // the host enqueues the whole run and synchronises once, at the end
    float* state_mem;
    TRY(ensure(c, c->stage[5], sizeof(OdState) / sizeof(float) + 16, &state_mem));
    OdState* state = reinterpret_cast<OdState*>(state_mem);
    const Mat4 init = load_T(odo_init);
    if (!c->od_host) HIPCHK(c, hipHostMalloc(&c->od_host, sizeof(OdState) + 64, hipHostMallocDefault));
    OdState* hst = reinterpret_cast<OdState*>(c->od_host);
    if (weighted) {  // the weighted variant's constants and its velocity, once
        std::memset(hst, 0, sizeof(OdState));
        hst->vel = I4;
        hst->sigma2 = option->sigma2_init;
        hst->nu = option->nu;
        for (int i = 0; i < 6; ++i) {
            hst->prev_twist[i] = prev_twist6 ? prev_twist6[i] : 0.0f;
            hst->inv_sigma[i] = option->inv_sigma_mat_diag[i];
        }
        HIPCHK(c, hipMemcpyAsync(state, hst, sizeof(OdState), hipMemcpyHostToDevice, c->stream));
    }
    // (two pinned slots: an asynchronous copy reads its host source when it executes, so the second
    // value must not overwrite the first one's source)
    Mat4* t_slots[2] = {&hst->T, reinterpret_cast<Mat4*>(reinterpret_cast<char*>(c->od_host) + sizeof(OdState))};
    int t_slot = 0;
    auto set_T = [&](const Mat4& T) -> int {
        Mat4* src = t_slots[t_slot++ & 1];
        *src = T;
        HIPCHK(c, hipMemcpyAsync(&state->T, src, sizeof(Mat4), hipMemcpyHostToDevice, c->stream));
        return MI_ICP_OK;
    };
    HIPCHK(c, hipMemsetAsync(sums, 0, 32 * sizeof(double), c->stream));
    OdArgs a{};
    a.out = sums;
    a.rows = rows;
    a.state = state;
    a.max_depth_diff = option->max_depth_diff;
    auto level_args = [&](int l) {
        a.depth_s = dep[0][l];
        a.depth_t = dep[1][l];
        a.color_s = col[0][l];
        a.color_t = col[1][l];
        a.dx_color = grad[0][l];
        a.dy_color = grad[1][l];
        a.dx_depth = grad[2][l];
        a.dy_depth = grad[3][l];
        a.w = lw[l];
        a.h = lh[l];
    };
    auto grid_for = [&](int l) {
        const int64_t n = (int64_t)lw[l] * lh[l];
        return (int)std::min<int64_t>(kOdMaxBlocks, std::max<int64_t>(1, (n + kOdThreads - 1) / kOdThreads));
    };
    // rows left by an evaluation of level l for whoever consumes its sums (0: it added to the totals itself)
    auto rows_of = [&](int l) { const int g = grid_for(l); return g > kOdAtomicBlocks ? g : 0; };
    {   // NormalizeIntensity (:416-436) over the correspondences under odo_init
        TRY(set_T(init));
        od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[0], 0, rows, 0);
        level_args(0);
        od_accumulate<kOdMeans><<<grid_for(0), kOdThreads, 0, c->stream>>>(a);
        if (rows_of(0)) od_total<<<1, kOdStepThreads, 0, c->stream>>>(rows, rows_of(0), sums);
        od_scale_by_mean<<<blocks(n0), kOdThreads, 0, c->stream>>>(col[0][0], n0, sums, 0);
        od_scale_by_mean<<<blocks(n0), kOdThreads, 0, c->stream>>>(col[1][0], n0, sums, 1);
        KCHK(c);
    }
    // ---- pyramids (rgbdimage.cu:96-112, image_factory.cu:251-278): colour Gaussian3 + Downsample,
    // depth Downsample only; Sobel3Dx / Sobel3Dy of the target per level (RGBDImage::FilterPyramid)
    for (int l = 1; l < L; ++l) {
        const int64_t np = (int64_t)lw[l - 1] * lh[l - 1], nn = (int64_t)lw[l] * lh[l];
        for (int s = 0; s < 2; ++s) {
            od_filter3<0, false><<<blocks(np), kOdThreads, 0, c->stream>>>(col[s][l - 1], lw[l - 1], lh[l - 1], scratch, 0.0f, 0.0f);
            od_downsample<<<blocks(nn), kOdThreads, 0, c->stream>>>(scratch, lw[l - 1], lh[l - 1], col[s][l]);
            od_downsample<<<blocks(nn), kOdThreads, 0, c->stream>>>(dep[s][l - 1], lw[l - 1], lh[l - 1], dep[s][l]);
        }
    }
    for (int l = 0; l < L; ++l) {
        const int64_t n = (int64_t)lw[l] * lh[l];
        od_filter3<1, false><<<blocks(n), kOdThreads, 0, c->stream>>>(col[1][l], lw[l], lh[l], grad[0][l], 0.0f, 0.0f);
        od_filter3<2, false><<<blocks(n), kOdThreads, 0, c->stream>>>(col[1][l], lw[l], lh[l], grad[1][l], 0.0f, 0.0f);
        od_filter3<1, false><<<blocks(n), kOdThreads, 0, c->stream>>>(dep[1][l], lw[l], lh[l], grad[2][l], 0.0f, 0.0f);
        od_filter3<2, false><<<blocks(n), kOdThreads, 0, c->stream>>>(dep[1][l], lw[l], lh[l], grad[3][l], 0.0f, 0.0f);
    }
    KCHK(c);

    // ---- ComputeMultiscale (:708-764): one accumulate + one step launch per iteration
    {
        bool zero = true;
        for (int i = 0; i < 16; ++i) zero = zero && (init.data()[i] == 0.0f);
        TRY(set_T(zero ? I4 : init));
        od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[L - 1], 0, rows, 0);  // terms for the coarsest level; zeroes the sums
    }
    for (int level = L - 1; level >= 0; --level) {
        level_args(level);
        const int iters = option->iterations[L - level - 1];
        for (int iter = 0; iter < iters; ++iter) {
            // the next evaluation: this level again, the next finer one, or level 0 (information matrix)
            const int next = (iter + 1 < iters) ? level : std::max(level - 1, 0);
            if (weighted) {  // two passes: the weights' normalisation, then the weighted system
                od_accumulate<kOdWeightSum><<<grid_for(level), kOdThreads, 0, c->stream>>>(a);
                od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[level], 3, rows, rows_of(level));
                od_accumulate<kOdWeighted><<<grid_for(level), kOdThreads, 0, c->stream>>>(a);
                od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[next], 2, rows, rows_of(level));
                continue;
            }
            if (jacobian == MI_ICP_ODOMETRY_COLOR_TERM) od_accumulate<kOdColor><<<grid_for(level), kOdThreads, 0, c->stream>>>(a);
            else od_accumulate<kOdHybrid><<<grid_for(level), kOdThreads, 0, c->stream>>>(a);
            od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[next], 1, rows, rows_of(level));
        }
        if (iters <= 0 && level > 0) od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[level - 1], 0, rows, 0);
    }
    KCHK(c);
    // CreateInformationMatrix (:349-394): I + sum G^T G over the final correspondences
    level_args(0);
    od_accumulate<kOdInformation><<<grid_for(0), kOdThreads, 0, c->stream>>>(a);
    if (rows_of(0)) od_total<<<1, kOdStepThreads, 0, c->stream>>>(rows, rows_of(0), sums);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->sys_host, sums, 32 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&hst->T, &state->T, sizeof(Mat4), hipMemcpyDeviceToHost, c->stream));
    if (weighted) HIPCHK(c, hipMemcpyAsync(&hst->vel, &state->vel, sizeof(Mat4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (weighted && twist6) od_matrix4_to_vector6(hst->vel, twist6);
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int q = r; q < 6; ++q, ++k) {
                information36[r * 6 + q] += c->sys_host[k];
                if (q != r) information36[q * 6 + r] += c->sys_host[k];
            }
        std::memcpy(transformation16, hst->T.data(), 16 * sizeof(float));
        *success = 1;  // without its determinant check the solver never reports failure (utility/eigen.cu:76-122)
    }
    for (int l = 0; l < L; ++l) {  // what mi_icp_debug_odometry_image hands out
        c->od_lw[l] = lw[l];
        c->od_lh[l] = lh[l];
        const float* img[8] = {col[0][l], dep[0][l], col[1][l], dep[1][l], grad[0][l], grad[1][l], grad[2][l], grad[3][l]};
        for (int k = 0; k < 8; ++k) c->od_img[l][k] = img[k];
    }
    c->od_levels = L;
    return MI_ICP_OK;
}

int mi_icp_compute_rgbd_odometry(mi_icp_ctx* c, const float* source_color, const float* source_depth,
                                 const float* target_color, const float* target_depth, int width, int height,
                                 const float* intrinsic4, const float* odo_init, int jacobian,
                                 const mi_icp_odometry_option* option, int* success, float* transformation16,
                                 double* information36, int mem_kind) {
    return rgbd_odometry_impl(c, source_color, source_depth, target_color, target_depth, width, height, intrinsic4,
                              odo_init, jacobian, option, success, transformation16, information36, mem_kind, false,
                              nullptr, nullptr);
}

int mi_icp_compute_weighted_rgbd_odometry(mi_icp_ctx* c, const float* source_color, const float* source_depth,
                                          const float* target_color, const float* target_depth, int width, int height,
                                          const float* intrinsic4, const float* odo_init, const float* prev_twist6,
                                          const mi_icp_odometry_option* option, int* success, float* transformation16,
                                          float* twist6, double* information36, int mem_kind) {
    if (!twist6) return c ? fail(c, MI_ICP_ERR_INVALID, "compute_weighted_rgbd_odometry: twist6 is null") : MI_ICP_ERR_INVALID;
    return rgbd_odometry_impl(c, source_color, source_depth, target_color, target_depth, width, height, intrinsic4,
                              odo_init, MI_ICP_ODOMETRY_HYBRID_TERM, option, success, transformation16, information36,
                              mem_kind, true, prev_twist6, twist6);
}

}  // extern "C"
