// cupoch_amd.cpp -- the C++ surface of cupoch's ICP path
// (namespace cupoch::{geometry,registration,utility}; headers under
// cupoch_amd/cpp/include/cupoch) implemented over libmi_icp.so's C ABI.
// Same names, defaults and error behaviour as the reference
// (registration/registration.cu:106-172, transformation_estimation.cu,
// generalized_icp.cu:37-61,185-198, geometry/pointcloud.cu:293-299,
// down_sample.cu:170-273, estimate_normals.cu:82-127); no kernel lives here.
#include <typeinfo>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <limits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>

#include "cupoch/cupoch.h"
#include "cupoch/utility/console.h"
#include "mi_icp.h"

namespace cupoch {

// ---------------------------------------------------------------- utility
namespace utility {

static void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        // the reference prints and exit(0)s (utility/platform.cu:60-67); throwing is the
        // closest well-behaved equivalent for a library
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    }
}
void* device_alloc(size_t bytes) {
    if (bytes == 0) return nullptr;
    void* p = nullptr;
    hip_check(hipMalloc(&p, bytes), "hipMalloc");
    return p;
}
void device_free(void* p) {
    if (p) (void)hipFree(p);
}
void copy_h2d(void* d, const void* s, size_t n) { hip_check(hipMemcpy(d, s, n, hipMemcpyHostToDevice), "hipMemcpy H2D"); }
void copy_d2h(void* d, const void* s, size_t n) { hip_check(hipMemcpy(d, s, n, hipMemcpyDeviceToHost), "hipMemcpy D2H"); }
void copy_d2d(void* d, const void* s, size_t n) { hip_check(hipMemcpy(d, s, n, hipMemcpyDeviceToDevice), "hipMemcpy D2D"); }

Eigen::Matrix4f TransformVector6fToMatrix4f(const Eigen::Vector6f& input) {
    Eigen::Matrix4f out;
    mi_icp_vector6_to_matrix4(input.data(), out.data());
    return out;
}

Eigen::Matrix4f InverseTransform(const Eigen::Matrix4f& input) {
    Eigen::Matrix4f inv = Eigen::Matrix4f::Identity();
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) inv(r, c) = input(c, r);
    for (int r = 0; r < 3; ++r)
        inv(r, 3) = -(inv(r, 0) * input(0, 3) + inv(r, 1) * input(1, 3) + inv(r, 2) * input(2, 3));
    return inv;
}

std::pair<bool, Eigen::Matrix4f> SolveJacobianSystemAndObtainExtrinsicMatrix(
        const Eigen::Matrix6f& JTJ, const Eigen::Vector6f& JTr, float det_thresh) {
    double sys[32] = {0};
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) sys[k++] = JTJ(i, j);
    for (int i = 0; i < 6; ++i) sys[21 + i] = JTr(i);
    Eigen::Matrix4f T;
    const int ok = mi_icp_solve_system(sys, det_thresh, T.data());
    return {ok > 0, T};
}

namespace {
VerbosityLevel g_verbosity = VerbosityLevel::Info;   // the reference's default (spdlog: info)
}
void SetVerbosityLevel(VerbosityLevel level) { g_verbosity = level; }
VerbosityLevel GetVerbosityLevel() { return g_verbosity; }

}  // namespace utility

// ---------------------------------------------------------------- engine
namespace {

void LogError(const char* msg) { std::fprintf(stderr, "[cupoch_amd] Error: %s\n", msg); }    // console.h:54-56: logs, continues
void LogWarning(const char* msg) { std::fprintf(stderr, "[cupoch_amd] Warning: %s\n", msg); }

mi_icp_ctx* Engine() {
    static mi_icp_ctx* ctx = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (mi_icp_create(dev, &ctx) != MI_ICP_OK)
            throw std::runtime_error("mi_icp_create failed: no MI355X device available (there is no CPU fallback)");
    });
    return ctx;
}

void Check(int rc) {
    if (rc < 0) throw std::runtime_error(std::string("mi_icp: ") + mi_icp_last_error(Engine()));
}

const float* Ptr(const utility::device_vector<Eigen::Vector3f>& v) { return v.empty() ? nullptr : v.data()->data(); }
const float* Ptr(const utility::device_vector<Eigen::Matrix3f>& v) { return v.empty() ? nullptr : v.data()->data(); }

// bumped whenever the engine's clouds are replaced: lets the generic ICP loop notice that a
// user estimator has used the engine (and that its own target tree / seeds are gone)
static unsigned long long g_load_generation = 0;

void LoadClouds(const geometry::PointCloud& source, const geometry::PointCloud& target) {
    mi_icp_ctx* c = Engine();
    ++g_load_generation;
    Check(mi_icp_set_target(c, Ptr(target.points_), target.HasNormals() ? Ptr(target.normals_) : nullptr,
                            target.HasCovariances() ? Ptr(target.covariances_) : nullptr,
                            (int64_t)target.points_.size(), MI_ICP_DEVICE));
    Check(mi_icp_set_source(c, Ptr(source.points_), source.HasNormals() ? Ptr(source.normals_) : nullptr,
                            source.HasCovariances() ? Ptr(source.covariances_) : nullptr,
                            (int64_t)source.points_.size(), MI_ICP_DEVICE));
}

registration::RegistrationResult MakeResult(const mi_icp_result& r) {
    registration::RegistrationResult out;
    std::memcpy(out.transformation_.data(), r.transformation, sizeof(float) * 16);
    out.fitness_ = r.fitness;
    out.inlier_rmse_ = r.inlier_rmse;
    int64_t count = 0;
    Check(mi_icp_get_correspondences(Engine(), nullptr, 0, &count, MI_ICP_DEVICE));
    out.correspondence_set_.resize((size_t)count);
    if (count > 0)
        Check(mi_icp_get_correspondences(Engine(), out.correspondence_set_.data()->data(), count, &count,
                                         MI_ICP_DEVICE));
    return out;
}

// estimator entry points on explicit correspondence sets
int EstType(registration::TransformationEstimationType t) { return (int)t; }

Eigen::Matrix4f ComputeWith(int est, float det_thresh, const geometry::PointCloud& source,
                            const geometry::PointCloud& target, const registration::CorrespondenceSet& corres) {
    if (corres.empty()) return Eigen::Matrix4f::Identity();
    LoadClouds(source, target);
    Check(mi_icp_set_correspondences(Engine(), corres.data()->data(), (int64_t)corres.size(), MI_ICP_DEVICE));
    Eigen::Matrix4f T;
    Check(mi_icp_compute_transformation(Engine(), est, nullptr, det_thresh, T.data()));
    return T;
}

float RmseWith(int est, const geometry::PointCloud& source, const geometry::PointCloud& target,
               const registration::CorrespondenceSet& corres) {
    if (corres.empty()) return 0.0f;
    LoadClouds(source, target);
    Check(mi_icp_set_correspondences(Engine(), corres.data()->data(), (int64_t)corres.size(), MI_ICP_DEVICE));
    float rmse = 0.0f;
    Check(mi_icp_compute_rmse(Engine(), est, nullptr, &rmse));
    return rmse;
}

}  // namespace

// ---------------------------------------------------------------- geometry
namespace geometry {

PointCloud& PointCloud::Transform(const Eigen::Matrix4f& transformation) {
    const size_t n = points_.size();
    Check(mi_icp_transform(Engine(), transformation.data(),
                           points_.empty() ? nullptr : points_.data()->data(),
                           normals_.size() == n && n ? normals_.data()->data() : nullptr,
                           covariances_.size() == n && n ? covariances_.data()->data() : nullptr,
                           (int64_t)n, MI_ICP_DEVICE));
    return *this;
}

std::shared_ptr<PointCloud> PointCloud::VoxelDownSample(float voxel_size) const {
    auto out = std::make_shared<PointCloud>();
    if (voxel_size <= 0.0f) {
        LogWarning("[VoxelDownSample] voxel_size <= 0.");  // down_sample.cu:173-176
        return out;
    }
    const size_t n = points_.size();
    if (n == 0) return out;
    const bool hn = HasNormals(), hc = HasColors();
    out->points_.resize(n);
    if (hn) out->normals_.resize(n);
    if (hc) out->colors_.resize(n);
    int64_t m = 0;
    Check(mi_icp_voxel_downsample(Engine(), Ptr(points_), hn ? Ptr(normals_) : nullptr,
                                  hc ? Ptr(colors_) : nullptr, (int64_t)n, voxel_size,
                                  out->points_.data()->data(), hn ? out->normals_.data()->data() : nullptr,
                                  hc ? out->colors_.data()->data() : nullptr, &m, MI_ICP_DEVICE));
    if (m == 0) LogWarning("[VoxelDownSample] voxel_size is too small.");
    out->points_.resize((size_t)m);
    if (hn) out->normals_.resize((size_t)m);
    if (hc) out->colors_.resize((size_t)m);
    return out;
}

// the output cloud of a selection: room for `rows` points (and normals / colours where this cloud has them)
static std::shared_ptr<PointCloud> SelectionOut(const PointCloud& pc, size_t rows) {
    auto out = std::make_shared<PointCloud>();
    out->points_.resize(rows);
    if (pc.HasNormals()) out->normals_.resize(rows);
    if (pc.HasColors()) out->colors_.resize(rows);
    return out;
}

static float* MutPtr(utility::device_vector<Eigen::Vector3f>& v) { return v.empty() ? nullptr : v.data()->data(); }

static void SelectionTrim(PointCloud& out, int64_t m) {
    out.points_.resize((size_t)m);
    if (!out.normals_.empty()) out.normals_.resize((size_t)m);
    if (!out.colors_.empty()) out.colors_.resize((size_t)m);
}

std::shared_ptr<PointCloud> PointCloud::SelectByIndex(const utility::device_vector<size_t>& indices, bool invert) const {
    const size_t n = points_.size();
    auto out = SelectionOut(*this, invert ? n : indices.size());
    int64_t m = 0;
    Check(mi_icp_select_by_index(Engine(), Ptr(points_), HasNormals() ? Ptr(normals_) : nullptr,
                                 HasColors() ? Ptr(colors_) : nullptr, (int64_t)n,
                                 (const int64_t*)indices.data(), (int64_t)indices.size(), invert ? 1 : 0,
                                 MutPtr(out->points_), MutPtr(out->normals_), MutPtr(out->colors_), &m, MI_ICP_DEVICE));
    SelectionTrim(*out, m);
    return out;
}

static_assert(sizeof(bool) == 1, "device_vector<bool> is handed to the engine as one byte per entry");

std::shared_ptr<PointCloud> PointCloud::SelectByMask(const utility::device_vector<bool>& mask, bool invert) const {
    const size_t n = points_.size();
    if (n != mask.size()) {  // down_sample.cu:134-137
        LogError("[SelectByMask] The point size should be equal to the mask size.");
        return std::make_shared<PointCloud>();
    }
    auto out = SelectionOut(*this, n);
    int64_t m = 0;
    Check(mi_icp_select_by_mask(Engine(), Ptr(points_), HasNormals() ? Ptr(normals_) : nullptr,
                                HasColors() ? Ptr(colors_) : nullptr, (int64_t)n, (const uint8_t*)mask.data(),
                                (int64_t)mask.size(), invert ? 1 : 0, MutPtr(out->points_), MutPtr(out->normals_),
                                MutPtr(out->colors_), &m, MI_ICP_DEVICE));
    SelectionTrim(*out, m);
    return out;
}

namespace keypoint {

std::tuple<std::shared_ptr<PointCloud>, std::shared_ptr<utility::device_vector<bool>>> ComputeISSKeypoints(
        const PointCloud& input, float salient_radius, float non_max_radius, float gamma_21, float gamma_32,
        int min_neighbors, int max_neighbors) {
    const size_t n = input.points_.size();
    if (n == 0) {  // iss_keypoints.cu:117-120
        LogWarning("[ComputeISSKeypoints] Input PointCloud is empty!");
        return std::make_tuple(std::make_shared<PointCloud>(), std::make_shared<utility::device_vector<bool>>());
    }
    auto mask = std::make_shared<utility::device_vector<bool>>(n);
    int64_t m = 0;
    Check(mi_icp_iss_keypoints(Engine(), Ptr(input.points_), (int64_t)n, salient_radius, non_max_radius, gamma_21,
                               gamma_32, min_neighbors, max_neighbors, (uint8_t*)mask->data(), nullptr, nullptr, nullptr,
                               nullptr, &m, MI_ICP_DEVICE));
    return std::make_tuple(input.SelectByMask(*mask), std::move(mask));
}

}  // namespace keypoint

std::shared_ptr<PointCloud> PointCloud::UniformDownSample(size_t every_k_points) const {
    if (every_k_points == 0) throw std::runtime_error("[UniformDownSample] Illegal sample rate.");  // down_sample.cu:277-280
    const size_t n = points_.size();
    auto out = SelectionOut(*this, n / every_k_points);
    int64_t m = 0;
    Check(mi_icp_uniform_downsample(Engine(), Ptr(points_), HasNormals() ? Ptr(normals_) : nullptr,
                                    HasColors() ? Ptr(colors_) : nullptr, (int64_t)n, (int64_t)every_k_points,
                                    MutPtr(out->points_), MutPtr(out->normals_), MutPtr(out->colors_), &m, MI_ICP_DEVICE));
    SelectionTrim(*out, m);
    return out;
}

// the two filters: the kept cloud and the kept points' indices, ascending
template <class Fn>
static std::tuple<std::shared_ptr<PointCloud>, utility::device_vector<size_t>> OutlierFilter(const PointCloud& pc, Fn fn) {
    const size_t n = pc.points_.size();
    auto out = SelectionOut(pc, n);
    utility::device_vector<size_t> idx(n);
    int64_t m = 0;
    Check(fn(pc.HasNormals() ? Ptr(pc.normals_) : nullptr, pc.HasColors() ? Ptr(pc.colors_) : nullptr, (int64_t)n,
             MutPtr(out->points_), MutPtr(out->normals_), MutPtr(out->colors_),
             n ? (int64_t*)idx.data() : nullptr, &m));
    SelectionTrim(*out, m);
    idx.resize((size_t)m);
    return std::make_tuple(out, std::move(idx));
}

static int CountArg(size_t v) { return v > 1000000 ? 1000000 : (int)v; }  // (anything above the limit is refused)

std::tuple<std::shared_ptr<PointCloud>, utility::device_vector<size_t>> PointCloud::RemoveRadiusOutliers(
        size_t nb_points, float search_radius) const {
    return OutlierFilter(*this, [&](const float* nrm, const float* col, int64_t n, float* op, float* on, float* oc,
                                    int64_t* idx, int64_t* m) {
        return mi_icp_remove_radius_outliers(Engine(), Ptr(points_), nrm, col, n, CountArg(nb_points), search_radius,
                                             op, on, oc, idx, nullptr, m, MI_ICP_DEVICE);
    });
}

std::tuple<std::shared_ptr<PointCloud>, utility::device_vector<size_t>> PointCloud::RemoveStatisticalOutliers(
        size_t nb_neighbors, float std_ratio) const {
    return OutlierFilter(*this, [&](const float* nrm, const float* col, int64_t n, float* op, float* on, float* oc,
                                    int64_t* idx, int64_t* m) {
        return mi_icp_remove_statistical_outliers(Engine(), Ptr(points_), nrm, col, n, CountArg(nb_neighbors), std_ratio,
                                                  op, on, oc, idx, nullptr, m, MI_ICP_DEVICE);
    });
}

std::shared_ptr<PointCloud> PointCloud::FarthestPointDownSample(size_t num_samples) const {
    const size_t n = points_.size();
    if (num_samples == 0) return std::make_shared<PointCloud>();
    if (num_samples > n) {  // pointcloud.cu:308-312
        LogError("[FarthestPointDownSample] Illegal number of samples, must <= point size.");
        return std::make_shared<PointCloud>();
    }
    auto out = SelectionOut(*this, num_samples);
    int64_t m = 0;
    Check(mi_icp_farthest_point_downsample(Engine(), Ptr(points_), HasNormals() ? Ptr(normals_) : nullptr,
                                           HasColors() ? Ptr(colors_) : nullptr, (int64_t)n, (int64_t)num_samples,
                                           MutPtr(out->points_), MutPtr(out->normals_), MutPtr(out->colors_), nullptr, &m,
                                           MI_ICP_DEVICE));
    SelectionTrim(*out, m);
    return out;
}

std::shared_ptr<PointCloud> PointCloud::GaussianFilter(float search_radius, float sigma2, size_t num_max_search_points) {
    if (!(search_radius > 0.0f) || !(sigma2 > 0.0f) || num_max_search_points == 0 ||
        num_max_search_points > (size_t)knn::NUM_MAX_NN) {  // pointcloud.cu:390-395
        LogError("[GaussianFilter] Illegal input parameters, radius and sigma2 must be positive.");
        return std::make_shared<PointCloud>();
    }
    const size_t n = points_.size();
    auto out = SelectionOut(*this, n);
    Check(mi_icp_gaussian_filter(Engine(), Ptr(points_), HasNormals() ? Ptr(normals_) : nullptr,
                                 HasColors() ? Ptr(colors_) : nullptr, (int64_t)n, search_radius, sigma2,
                                 (int)num_max_search_points, MutPtr(out->points_), MutPtr(out->normals_),
                                 MutPtr(out->colors_), MI_ICP_DEVICE));
    return out;
}

// the three predicate filters: the kept cloud
template <class Fn>
static std::shared_ptr<PointCloud> PredicateFilter(const PointCloud& pc, Fn fn) {
    const size_t n = pc.points_.size();
    auto out = SelectionOut(pc, n);
    int64_t m = 0;
    Check(fn(pc.HasNormals() ? Ptr(pc.normals_) : nullptr, pc.HasColors() ? Ptr(pc.colors_) : nullptr, (int64_t)n,
             MutPtr(out->points_), MutPtr(out->normals_), MutPtr(out->colors_), &m));
    SelectionTrim(*out, m);
    return out;
}

std::shared_ptr<PointCloud> PointCloud::PassThroughFilter(size_t axis_no, float min_bound, float max_bound) {
    if (axis_no >= 3) {  // pointcloud.cu:440-445
        LogError("[PassThroughFilter] Illegal input parameters, axis_no must be 0, 1 or 2.");
        return std::make_shared<PointCloud>();
    }
    return PredicateFilter(*this, [&](const float* nrm, const float* col, int64_t n, float* op, float* on, float* oc, int64_t* m) {
        return mi_icp_pass_through_filter(Engine(), Ptr(points_), nrm, col, n, (int)axis_no, min_bound, max_bound, op, on, oc,
                                          nullptr, m, MI_ICP_DEVICE);
    });
}

std::shared_ptr<PointCloud> PointCloud::Crop(const AxisAlignedBoundingBox3& bbox) const {
    if (!(bbox.Volume() > 0.0f)) {  // pointcloud.cu:342-346
        LogError("[CropPointCloud] AxisAlignedBoundingBox either has zeros size, or has wrong bounds.");
        return std::make_shared<PointCloud>();
    }
    return PredicateFilter(*this, [&](const float* nrm, const float* col, int64_t n, float* op, float* on, float* oc, int64_t* m) {
        return mi_icp_crop_aabb(Engine(), Ptr(points_), nrm, col, n, bbox.min_bound_.data(), bbox.max_bound_.data(), op, on,
                                oc, nullptr, m, MI_ICP_DEVICE);
    });
}

PointCloud& PointCloud::RemoveNoneFinitePoints(bool remove_nan, bool remove_infinite) {
    const bool hn = HasNormals(), hc = HasColors();
    auto kept = PredicateFilter(*this, [&](const float* nrm, const float* col, int64_t n, float* op, float* on, float* oc, int64_t* m) {
        return mi_icp_remove_none_finite(Engine(), Ptr(points_), nrm, col, n, remove_nan ? 1 : 0, remove_infinite ? 1 : 0, op,
                                         on, oc, nullptr, m, MI_ICP_DEVICE);
    });
    if (kept->points_.size() != points_.size()) covariances_.clear();  // (not carried, in the reference neither)
    points_.swap(kept->points_);
    if (hn) normals_.swap(kept->normals_);
    if (hc) colors_.swap(kept->colors_);
    return *this;
}

std::unique_ptr<utility::device_vector<int>> PointCloud::ClusterDBSCAN(float eps, size_t min_points, bool,
                                                                       size_t max_edges) const {
    const size_t n = points_.size();
    auto labels = std::make_unique<utility::device_vector<int>>(n);
    int64_t n_clusters = 0;
    Check(mi_icp_cluster_dbscan(Engine(), Ptr(points_), (int64_t)n, eps,
                                (int64_t)std::min<size_t>(min_points, (size_t)1 << 40),  // (all that large mean "no core")
                                CountArg(max_edges), n ? labels->data() : nullptr, nullptr, &n_clusters, MI_ICP_DEVICE));
    return labels;
}

std::tuple<Eigen::Vector4f, utility::device_vector<size_t>> PointCloud::SegmentPlane(float distance_threshold, size_t ransac_n,
                                                                                      size_t num_iterations) const {
    Eigen::Vector4f plane;
    for (int k = 0; k < 4; ++k) plane(k) = 0.0f;
    utility::device_vector<size_t> inliers;
    const size_t n = points_.size();
    if (ransac_n < 3) {  // segmentation.cu:204-212
        LogError("ransac_n should be set to higher than or equal to 3.");
        return std::make_tuple(plane, std::move(inliers));
    }
    if (n < ransac_n) {
        LogError("There must be at least 'ransac_n' points.");
        return std::make_tuple(plane, std::move(inliers));
    }
    inliers.resize(n);
    int64_t m = 0;
    const uint64_t seed = (uint64_t)std::rand();
    Check(mi_icp_segment_plane(Engine(), Ptr(points_), (int64_t)n, distance_threshold, (int64_t)ransac_n,
                               (int64_t)std::min<size_t>(num_iterations, (size_t)1 << 40), seed, plane.data(), nullptr,
                               (int64_t*)inliers.data(), &m, nullptr, nullptr, MI_ICP_DEVICE));
    inliers.resize((size_t)m);
    return std::make_tuple(plane, std::move(inliers));
}

bool PointCloud::EstimateNormals(const knn::KDTreeSearchParam& search_param) {
    normals_.resize(points_.size());
    if (points_.empty()) return true;
    switch (search_param.GetSearchType()) {
        case knn::KDTreeSearchParam::SearchType::Knn:
            Check(mi_icp_estimate_normals_knn(Engine(), Ptr(points_), (int64_t)points_.size(),
                                              ((const knn::KDTreeSearchParamKNN&)search_param).knn_,
                                              normals_.data()->data(), MI_ICP_DEVICE));
            return true;
        case knn::KDTreeSearchParam::SearchType::Radius: {
            const auto& p = (const knn::KDTreeSearchParamRadius&)search_param;
            Check(mi_icp_estimate_normals_radius(Engine(), Ptr(points_), (int64_t)points_.size(), p.radius_,
                                                 p.max_nn_, normals_.data()->data(), MI_ICP_DEVICE));
            return true;
        }
        default:
            LogError("Unknown search param type.");  // estimate_normals.cu:102-104
            return false;
    }
}

// GeometryBase3D on a cloud (pointcloud.cu:205-242): device reductions / one in-place kernel each
static void Bounds(const utility::device_vector<Eigen::Vector3f>& pts, Eigen::Vector3f* mn, Eigen::Vector3f* mx,
                   Eigen::Vector3f* center) {
    Check(mi_icp_compute_bounds(Engine(), Ptr(pts), (int64_t)pts.size(), MI_ICP_DEVICE, mn ? mn->data() : nullptr,
                                mx ? mx->data() : nullptr, center ? center->data() : nullptr));
}
Eigen::Vector3f PointCloud::GetMinBound() const {
    Eigen::Vector3f b;
    Bounds(points_, &b, nullptr, nullptr);
    return b;
}
Eigen::Vector3f PointCloud::GetMaxBound() const {
    Eigen::Vector3f b;
    Bounds(points_, nullptr, &b, nullptr);
    return b;
}
Eigen::Vector3f PointCloud::GetCenter() const {
    Eigen::Vector3f b;
    Bounds(points_, nullptr, nullptr, &b);
    return b;
}
AxisAlignedBoundingBox3 PointCloud::GetAxisAlignedBoundingBox() const {  // AxisAlignedBoundingBox<3>::CreateFromPoints
    Eigen::Vector3f mn, mx;
    Bounds(points_, &mn, &mx, nullptr);
    return AxisAlignedBoundingBox3(mn, mx);
}
PointCloud& PointCloud::Translate(const Eigen::Vector3f& translation, bool relative) {
    Eigen::Vector3f t = translation;
    if (!relative) t -= GetCenter();                       // geometry_utils.cu:155-158
    Check(mi_icp_affine(Engine(), nullptr, 0.0f, 0, nullptr, t.data(), points_.empty() ? nullptr : points_.data()->data(),
                        nullptr, nullptr, (int64_t)points_.size(), MI_ICP_DEVICE));
    return *this;
}
PointCloud& PointCloud::Scale(const float scale, bool center) {
    Eigen::Vector3f c = Eigen::Vector3f::Zero();
    const bool use_c = center && !points_.empty();          // geometry_utils.cu:170-173
    if (use_c) c = GetCenter();
    Check(mi_icp_affine(Engine(), nullptr, scale, 1, use_c ? c.data() : nullptr, nullptr,
                        points_.empty() ? nullptr : points_.data()->data(), nullptr, nullptr, (int64_t)points_.size(),
                        MI_ICP_DEVICE));
    return *this;
}
PointCloud& PointCloud::Rotate(const Eigen::Matrix3f& R, bool center) {
    Eigen::Vector3f c = Eigen::Vector3f::Zero();
    const bool use_c = center && !points_.empty();          // geometry_utils.cu:211-214
    if (use_c) c = GetCenter();
    const size_t n = points_.size();
    Check(mi_icp_affine(Engine(), R.data(), 0.0f, 0, use_c ? c.data() : nullptr, nullptr,
                        n ? points_.data()->data() : nullptr, normals_.size() == n && n ? normals_.data()->data() : nullptr,
                        covariances_.size() == n && n ? covariances_.data()->data() : nullptr, (int64_t)n,
                        MI_ICP_DEVICE));
    return *this;
}

// geometry::AxisAlignedBoundingBox<3> (geometry/boundingvolume.cu:300-354)
AxisAlignedBoundingBox3 AxisAlignedBoundingBox3::GetAxisAlignedBoundingBox() const { return *this; }
AxisAlignedBoundingBox3& AxisAlignedBoundingBox3::Transform(const Eigen::Matrix4f&) {
    LogError("A general transform of a AxisAlignedBoundingBox would not be axis aligned anymore, convert it to a "
             "OrientedBoundingBox first");
    return *this;
}
AxisAlignedBoundingBox3& AxisAlignedBoundingBox3::Translate(const Eigen::Vector3f& translation, bool relative) {
    if (relative) {
        min_bound_ += translation;
        max_bound_ += translation;
    } else {
        const Eigen::Vector3f half_extent = GetHalfExtent();
        min_bound_ = translation - half_extent;
        max_bound_ = translation + half_extent;
    }
    return *this;
}
AxisAlignedBoundingBox3& AxisAlignedBoundingBox3::Scale(const float scale, bool center) {
    if (center) {
        const Eigen::Vector3f c = GetCenter();
        min_bound_ = c + scale * (min_bound_ - c);
        max_bound_ = c + scale * (max_bound_ - c);
    } else {
        min_bound_ *= scale;
        max_bound_ *= scale;
    }
    return *this;
}
AxisAlignedBoundingBox3& AxisAlignedBoundingBox3::Rotate(const Eigen::Matrix3f&, bool) {
    LogError("A rotation of a AxisAlignedBoundingBox would not be axis aligned anymore, convert it to an "
             "OrientedBoundingBox first");
    return *this;
}

static std::shared_ptr<PointCloud> FromDepth(const Image& depth, const Image* color, int color_type,
                                             const camera::PinholeCameraIntrinsic& intrinsic,
                                             const Eigen::Matrix4f& extrinsic, float depth_scale, float depth_trunc,
                                             float depth_cutoff, int stride, bool rgbd, bool compute_normals,
                                             bool valid_only) {
    auto out = std::make_shared<PointCloud>();
    if (stride < 1 || depth.width_ <= 0 || depth.height_ <= 0) return out;
    const size_t count = (size_t)(depth.width_ / stride) * (size_t)(depth.height_ / stride);
    if (count == 0) return out;
    out->points_.resize(count);
    if (color) out->colors_.resize(count);
    if (compute_normals) out->normals_.resize(count);
    const float k4[4] = {intrinsic.fx_, intrinsic.fy_, intrinsic.cx_, intrinsic.cy_};
    int64_t m = 0;
    Check(mi_icp_create_from_depth(Engine(), depth.data_.data(),
                                   depth.bytes_per_channel_ == 2 ? MI_ICP_DEPTH_U16 : MI_ICP_DEPTH_F32,
                                   color ? color->data_.data() : nullptr, color_type, depth.width_, depth.height_, k4,
                                   extrinsic.data(), depth_scale, depth_trunc, depth_cutoff, stride, rgbd ? 1 : 0,
                                   compute_normals ? 1 : 0, valid_only ? 1 : 0, out->points_.data()->data(),
                                   compute_normals ? out->normals_.data()->data() : nullptr,
                                   color ? out->colors_.data()->data() : nullptr, &m, MI_ICP_DEVICE));
    out->points_.resize((size_t)m);
    if (color) out->colors_.resize((size_t)m);
    if (compute_normals) out->normals_.resize((size_t)m);
    return out;
}

std::shared_ptr<PointCloud> PointCloud::CreateFromDepthImage(const Image& depth,
                                                             const camera::PinholeCameraIntrinsic& intrinsic,
                                                             const Eigen::Matrix4f& extrinsic, float depth_scale,
                                                             float depth_trunc, int stride) {
    if (depth.num_of_channels_ == 1 && (depth.bytes_per_channel_ == 2 || depth.bytes_per_channel_ == 4))
        return FromDepth(depth, nullptr, MI_ICP_COLOR_NONE, intrinsic, extrinsic, depth_scale, depth_trunc, -1.0f,
                         stride, false, false, true);
    LogError("[PointCloud::CreateFromDepthImage] Unsupported image format.");  // pointcloud_factory.cu:348-350
    return std::make_shared<PointCloud>();
}

std::shared_ptr<PointCloud> PointCloud::CreateFromRGBDImage(const RGBDImage& image,
                                                            const camera::PinholeCameraIntrinsic& intrinsic,
                                                            const Eigen::Matrix4f& extrinsic,
                                                            bool project_valid_depth_only, float depth_cutoff,
                                                            bool compute_normals) {
    const Image& c = image.color_;
    const bool depth_ok = image.depth_.num_of_channels_ == 1 && image.depth_.bytes_per_channel_ == 4;
    int color_type = -1;
    if (c.data_.empty()) color_type = MI_ICP_COLOR_NONE;
    else if (c.bytes_per_channel_ == 1 && c.num_of_channels_ == 3) color_type = MI_ICP_COLOR_U8X3;
    else if (c.bytes_per_channel_ == 4 && c.num_of_channels_ == 1) color_type = MI_ICP_COLOR_F32X1;
    if (!depth_ok || color_type < 0 ||
        (color_type != MI_ICP_COLOR_NONE && (c.width_ != image.depth_.width_ || c.height_ != image.depth_.height_))) {
        LogError("[PointCloud::CreateFromRGBDImage] Unsupported image format.");  // pointcloud_factory.cu:373-375
        return std::make_shared<PointCloud>();
    }
    return FromDepth(image.depth_, color_type == MI_ICP_COLOR_NONE ? nullptr : &c, color_type, intrinsic, extrinsic,
                     1000.0f, 1000.0f, depth_cutoff, 1, true, compute_normals, project_valid_depth_only);
}

std::shared_ptr<PointCloud> PointCloud::CreateFromDisparity(const Image& disp, const Image& color,
                                                            const camera::PinholeCameraIntrinsic& left_intrinsic,
                                                            const camera::PinholeCameraIntrinsic& right_intrinsic,
                                                            float baseline) {
    auto out = std::make_shared<PointCloud>();
    if (!(disp.num_of_channels_ == 1 && disp.bytes_per_channel_ == 1 && disp.width_ == color.width_ &&
          disp.height_ == color.height_ && color.num_of_channels_ == 3 &&
          (color.bytes_per_channel_ == 1 || color.bytes_per_channel_ == 2))) {
        LogError("[PointCloud::CreateFromDisparity] Unsupported image format.");  // pointcloud_factory.cu:479-481
        return out;
    }
    const float tx = -baseline;
    const auto f = left_intrinsic.GetFocalLength();
    const auto pl = left_intrinsic.GetPrincipalPoint();
    const auto pr = right_intrinsic.GetPrincipalPoint();
    // pointcloud_factory.cu:444-455, every product and difference rounded to float in the order written
    volatile float q[7];
    q[0] = f.second * tx;
    q[1] = -f.second * pl.first;
    q[1] = q[1] * tx;
    q[2] = f.first * tx;
    q[3] = -f.first * pl.second;
    q[3] = q[3] * tx;
    q[4] = f.first * f.second;
    q[4] = q[4] * tx;
    q[5] = -f.second;
    q[6] = pl.first - pr.first;
    q[6] = f.second * q[6];
    const float qs[7] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6]};
    const size_t n = (size_t)disp.width_ * (size_t)disp.height_;
    out->points_.resize(n);
    out->colors_.resize(n);
    if (n == 0) return out;
    Check(mi_icp_create_from_disparity(Engine(), disp.data_.data(), color.data_.data(), disp.width_, disp.height_,
                                       color.bytes_per_channel_, qs, out->points_.data()->data(), out->colors_.data()->data()));
    return out;
}

}  // namespace geometry

// ---------------------------------------------------------------- imageproc
namespace imageproc {

SemiGlobalMatching::SemiGlobalMatching(const SGMOption& option) : option_(option) {
    const SGMOption& o = option_;
    if (o.width_ <= 0 || o.height_ <= 0) {   // (before any engine: no device is needed to be turned away)
        LogError("[SemiGlobalMatching::SemiGlobalMatching] Invalid SGM parameters: width and height must be positive.");
        return;
    }
    const int rc = mi_icp_sgm_create(Engine(), o.width_, o.height_, o.p1_, o.p2_, o.uniqueness_, (int)o.disp_size_,
                                     (int)o.path_type_, o.min_disp_, o.lr_max_diff_, &matcher_);
    if (rc == MI_ICP_ERR_INVALID) {
        LogError((std::string("[SemiGlobalMatching::SemiGlobalMatching] Invalid SGM parameters: ") + mi_icp_last_error(Engine())).c_str());
        matcher_ = nullptr;
        return;
    }
    Check(rc);
}

SemiGlobalMatching::~SemiGlobalMatching() {
    if (matcher_) (void)mi_icp_sgm_destroy(Engine(), matcher_);
}

std::shared_ptr<geometry::Image> SemiGlobalMatching::ProcessFrame(const geometry::Image& left, const geometry::Image& right) {
    auto output = std::make_shared<geometry::Image>();
    if (!matcher_) {
        LogError("[SemiGlobalMatching::ProcessFrame] Invalid SGM parameters.");  // sgm.cpp:49-53
        return output;
    }
    if (left.width_ != option_.width_ || left.height_ != option_.height_ || right.width_ != option_.width_ ||
        right.height_ != option_.height_ || left.num_of_channels_ != 1 || right.num_of_channels_ != 1 ||
        left.bytes_per_channel_ != 1 || right.bytes_per_channel_ != 1) {
        LogError("[SemiGlobalMatching::ProcessFrame] Unsupport image type.");  // sgm.cpp:54-60
        return output;
    }
    output->Prepare(left.width_, left.height_, 1, 1);
    Check(mi_icp_sgm_process(Engine(), matcher_, left.data_.data(), right.data_.data(), output->data_.data()));
    return output;
}

}  // namespace imageproc

// ---------------------------------------------------------------- registration
namespace registration {

float TransformationEstimationPointToPoint::ComputeRMSE(const geometry::PointCloud& s, const geometry::PointCloud& t,
                                                        const CorrespondenceSet& c) const {
    return RmseWith(MI_ICP_EST_POINT_TO_POINT, s, t, c);
}
Eigen::Matrix4f TransformationEstimationPointToPoint::ComputeTransformation(const geometry::PointCloud& s,
                                                                            const geometry::PointCloud& t,
                                                                            const CorrespondenceSet& c) const {
    return ComputeWith(MI_ICP_EST_POINT_TO_POINT, -1.0f, s, t, c);
}
float TransformationEstimationPointToPlane::ComputeRMSE(const geometry::PointCloud& s, const geometry::PointCloud& t,
                                                        const CorrespondenceSet& c) const {
    if (!t.HasNormals()) return 0.0f;
    return RmseWith(MI_ICP_EST_POINT_TO_PLANE, s, t, c);
}
Eigen::Matrix4f TransformationEstimationPointToPlane::ComputeTransformation(const geometry::PointCloud& s,
                                                                            const geometry::PointCloud& t,
                                                                            const CorrespondenceSet& c) const {
    if (!t.HasNormals()) return Eigen::Matrix4f::Identity();
    return ComputeWith(MI_ICP_EST_POINT_TO_PLANE, det_thresh_, s, t, c);
}
float TransformationEstimationSymmetricMethod::ComputeRMSE(const geometry::PointCloud& s, const geometry::PointCloud& t,
                                                           const CorrespondenceSet& c) const {
    if (!s.HasNormals() || !t.HasNormals()) return 0.0f;
    return RmseWith(MI_ICP_EST_SYMMETRIC, s, t, c);
}
Eigen::Matrix4f TransformationEstimationSymmetricMethod::ComputeTransformation(const geometry::PointCloud& s,
                                                                               const geometry::PointCloud& t,
                                                                               const CorrespondenceSet& c) const {
    if (!s.HasNormals() || !t.HasNormals()) return Eigen::Matrix4f::Identity();
    return ComputeWith(MI_ICP_EST_SYMMETRIC, det_thresh_, s, t, c);
}
float TransformationEstimationForGeneralizedICP::ComputeRMSE(const geometry::PointCloud& s,
                                                             const geometry::PointCloud& t,
                                                             const CorrespondenceSet& c) const {
    if (!s.HasCovariances() || !t.HasCovariances()) return 0.0f;
    return RmseWith(MI_ICP_EST_GENERALIZED, s, t, c);
}
Eigen::Matrix4f TransformationEstimationForGeneralizedICP::ComputeTransformation(const geometry::PointCloud& s,
                                                                                 const geometry::PointCloud& t,
                                                                                 const CorrespondenceSet& c) const {
    if (!s.HasCovariances() || !t.HasCovariances()) return Eigen::Matrix4f::Identity();
    return ComputeWith(MI_ICP_EST_GENERALIZED, -1.0f, s, t, c);
}

RegistrationResult EvaluateRegistration(const geometry::PointCloud& source, const geometry::PointCloud& target,
                                        float max_correspondence_distance, const Eigen::Matrix4f& transformation) {
    LoadClouds(source, target);
    mi_icp_result r;
    Check(mi_icp_evaluate_registration(Engine(), max_correspondence_distance, transformation.data(), &r));
    return MakeResult(r);
}

// exact type, not dynamic_cast: a user subclass of a built-in estimator may override
// ComputeTransformation, and the reference always makes the virtual call (registration.cu:157)
static bool IsBuiltin(const TransformationEstimation& e) {
    const std::type_info& t = typeid(e);
    return t == typeid(TransformationEstimationPointToPoint) || t == typeid(TransformationEstimationPointToPlane) ||
           t == typeid(TransformationEstimationSymmetricMethod) ||
           t == typeid(TransformationEstimationForGeneralizedICP);
}

RegistrationResult RegistrationICP(const geometry::PointCloud& source, const geometry::PointCloud& target,
                                   float max_correspondence_distance, const Eigen::Matrix4f& init,
                                   const TransformationEstimation& estimation,
                                   const ICPConvergenceCriteria& criteria) {
    if (max_correspondence_distance <= 0.0f) LogError("Invalid max_correspondence_distance.");  // registration.cu:130-132
    const auto type = estimation.GetTransformationEstimationType();
    if ((type == TransformationEstimationType::PointToPlane || type == TransformationEstimationType::ColoredICP) &&
        !target.HasNormals())
        LogError("TransformationEstimationPointToPlane and TransformationEstimationColoredICP require "
                 "pre-computed target normal vectors.");  // registration.cu:134-143

    if (IsBuiltin(estimation)) {  // fused device loop
        float det = -1.0f;
        if (auto* p = dynamic_cast<const TransformationEstimationPointToPlane*>(&estimation)) det = p->det_thresh_;
        if (auto* p = dynamic_cast<const TransformationEstimationSymmetricMethod*>(&estimation)) det = p->det_thresh_;
        LoadClouds(source, target);
        mi_icp_params prm = {criteria.relative_fitness_, criteria.relative_rmse_, criteria.max_iteration_, det};
        mi_icp_result r;
        // utility::LogDebug("ICP Iteration #{:d}: Fitness {:.4f}, RMSE {:.4f}", ...) (registration.cu:155-156)
        const bool debug = utility::GetVerbosityLevel() <= utility::VerbosityLevel::Debug;
        if (debug)
            mi_icp_set_iteration_callback(Engine(), [](void*, int i, float fitness, float rmse) {
                std::fprintf(stderr, "[cupoch_amd] Debug: ICP Iteration #%d: Fitness %.4f, RMSE %.4f\n", i, fitness, rmse);
            }, nullptr);
        const int rc = mi_icp_registration_icp(Engine(), EstType(type), max_correspondence_distance, init.data(), &prm, &r);
        if (debug) mi_icp_set_iteration_callback(Engine(), nullptr, nullptr);
        Check(rc);
        return MakeResult(r);
    }

    // user-defined estimator: the reference loop (registration.cu:144-171).  The engine keeps the
    // ORIGINAL source and the target tree and evaluates under the accumulated transformation
    // (seeded by the previous iteration's matches); the estimator still sees the transformed copy.
    // If the estimator itself goes through the engine, the clouds are simply loaded again.
    Eigen::Matrix4f transformation = init;
    geometry::PointCloud pcd = source;
    if (!init.isIdentity()) pcd.Transform(init);
    unsigned long long loaded = 0;
    auto evaluate = [&](const Eigen::Matrix4f& T) {
        if (loaded == 0 || loaded != g_load_generation) {
            LoadClouds(source, target);
            loaded = g_load_generation;
        }
        mi_icp_result r;
        Check(mi_icp_evaluate_registration(Engine(), max_correspondence_distance, T.data(), &r));
        RegistrationResult res = MakeResult(r);
        res.transformation_ = T;
        return res;
    };
    RegistrationResult result = evaluate(transformation);
    for (int i = 0; i < criteria.max_iteration_; ++i) {
        const Eigen::Matrix4f update = estimation.ComputeTransformation(pcd, target, result.correspondence_set_);
        transformation = update * transformation;
        pcd.Transform(update);
        RegistrationResult backup = result;
        result = evaluate(transformation);
        if (std::fabs(backup.fitness_ - result.fitness_) < criteria.relative_fitness_ &&
            std::fabs(backup.inlier_rmse_ - result.inlier_rmse_) < criteria.relative_rmse_)
            break;
    }
    return result;
}

// InitializePointCloudForGeneralizedICP (generalized_icp.cu:37-61)
static std::shared_ptr<geometry::PointCloud> InitializeForGICP(const geometry::PointCloud& pcd, float epsilon) {
    auto out = std::make_shared<geometry::PointCloud>(pcd);
    if (out->HasCovariances()) return out;
    if (!out->HasNormals()) out->EstimateNormals(knn::KDTreeSearchParamKNN(20));
    out->covariances_.resize(out->points_.size());
    if (!out->points_.empty())
        Check(mi_icp_covariances_from_normals(Engine(), Ptr(out->normals_), (int64_t)out->points_.size(), epsilon,
                                              out->covariances_.data()->data(), MI_ICP_DEVICE));
    return out;
}

RegistrationResult RegistrationGeneralizedICP(const geometry::PointCloud& source, const geometry::PointCloud& target,
                                              float max_correspondence_distance, const Eigen::Matrix4f& init,
                                              const TransformationEstimationForGeneralizedICP& estimation,
                                              const ICPConvergenceCriteria& criteria) {
    return RegistrationICP(*InitializeForGICP(source, estimation.epsilon_), *InitializeForGICP(target, estimation.epsilon_),
                           max_correspondence_distance, init, estimation, criteria);
}

// registration::RegistrationColoredICP (colored_icp.cu:329-341)
RegistrationResult RegistrationColoredICP(const geometry::PointCloud& source, const geometry::PointCloud& target,
                                          float max_distance, const Eigen::Matrix4f& init,
                                          const ICPConvergenceCriteria& criteria, float lambda_geometric,
                                          float det_thresh) {
    if (max_distance <= 0.0f) LogError("Invalid max_correspondence_distance.");
    if (!target.HasNormals())
        LogError("TransformationEstimationPointToPlane and TransformationEstimationColoredICP require "
                 "pre-computed target normal vectors.");
    LoadClouds(source, target);
    if (target.HasNormals() && target.HasColors())
        Check(mi_icp_set_target_colors(Engine(), Ptr(target.colors_), MI_ICP_DEVICE));
    if (source.HasColors()) Check(mi_icp_set_source_colors(Engine(), Ptr(source.colors_), MI_ICP_DEVICE));
    mi_icp_params prm = {criteria.relative_fitness_, criteria.relative_rmse_, criteria.max_iteration_, det_thresh};
    mi_icp_result r;
    Check(mi_icp_registration_colored_icp(Engine(), max_distance, init.data(), &prm, lambda_geometric, &r));
    return MakeResult(r);
}

Eigen::Matrix4f_u Kabsch(const utility::device_vector<Eigen::Vector3f>& model,
                         const utility::device_vector<Eigen::Vector3f>& target) {
    // all points paired by index (kabsch.cu:122-): an identity correspondence set
    const size_t n = model.size();
    std::vector<Eigen::Vector2i> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = Eigen::Vector2i((int)i, (int)i);
    CorrespondenceSet corres(h);
    geometry::PointCloud s, t;
    s.points_ = model;
    t.points_ = target;
    return ComputeWith(MI_ICP_EST_POINT_TO_POINT, -1.0f, s, t, corres);
}

// registration::CorrespondencesFromFeatures / FastGlobalRegistration (include/mi_icp.h "feature matching and
// FastGlobalRegistration"); a Feature's data_ is [Num()][Dim] floats, the layout the C ABI takes
template <int Dim>
CorrespondenceSet CorrespondencesFromFeatures(const Feature<Dim>& source_features, const Feature<Dim>& target_features,
                                              bool mutual_filter, float mutual_consistency_ratio) {
    CorrespondenceSet out;
    if (source_features.IsEmpty() || target_features.IsEmpty()) return out;
    out.resize(source_features.Num());
    int64_t m = 0;
    Check(mi_icp_correspondences_from_features(Engine(), source_features.data_.data()->data(), (int64_t)source_features.Num(),
                                               target_features.data_.data()->data(), (int64_t)target_features.Num(), Dim,
                                               mutual_filter ? 1 : 0, mutual_consistency_ratio, out.data()->data(), &m));
    out.resize((size_t)m);
    return out;
}

template <int Dim>
RegistrationResult FastGlobalRegistration(const geometry::PointCloud& source, const geometry::PointCloud& target,
                                          const Feature<Dim>& source_feature, const Feature<Dim>& target_feature,
                                          const FastGlobalRegistrationOption& option, uint64_t seed) {
    if (!source.HasPoints() || !target.HasPoints() || source_feature.IsEmpty() || target_feature.IsEmpty()) {
        LogError("Invalid source or target pointcloud.");  // fast_global_registration.cu:401-405
        return RegistrationResult();
    }
    if (source_feature.Num() != source.points_.size() || target_feature.Num() != target.points_.size())
        throw std::runtime_error("FastGlobalRegistration: one descriptor per point is needed");
    const mi_icp_fgr_option o = {option.division_factor_, option.use_absolute_scale_ ? 1 : 0, option.decrease_mu_ ? 1 : 0,
                                 option.maximum_correspondence_distance_, option.iteration_number_, option.tuple_scale_,
                                 option.maximum_tuple_count_};
    ++g_load_generation;  // (the call loads both clouds for its EvaluateRegistration)
    mi_icp_result r;
    Check(mi_icp_fast_global_registration(Engine(), Ptr(source.points_), source_feature.data_.data()->data(),
                                          (int64_t)source.points_.size(), Ptr(target.points_), target_feature.data_.data()->data(),
                                          (int64_t)target.points_.size(), Dim, &o, seed, &r));
    return MakeResult(r);
}

#define CUPOCH_AMD_FEATURE_DIM(Dim)                                                                                               \
    template CorrespondenceSet CorrespondencesFromFeatures<Dim>(const Feature<Dim>&, const Feature<Dim>&, bool, float);           \
    template RegistrationResult FastGlobalRegistration<Dim>(const geometry::PointCloud&, const geometry::PointCloud&,             \
                                                            const Feature<Dim>&, const Feature<Dim>&,                             \
                                                            const FastGlobalRegistrationOption&, uint64_t);
CUPOCH_AMD_FEATURE_DIM(33)
CUPOCH_AMD_FEATURE_DIM(352)
#undef CUPOCH_AMD_FEATURE_DIM

}  // namespace registration
// ============================================================================
// knn::BruteForceNN (knn/bruteforce_nn.h), knn::KDTreeFlann (knn/kdtree_flann.h:43-124)
// ============================================================================
namespace knn {

template <int Dim>
void BruteForceNN(const utility::device_vector<Eigen::Matrix<float, Dim, 1>>& ref,
                  const utility::device_vector<Eigen::Matrix<float, Dim, 1>>& query, utility::device_vector<int>& indices,
                  utility::device_vector<float>& distances) {
    indices.resize(query.size());
    distances.resize(query.size());
    if (query.empty()) return;
    if (ref.empty()) throw std::runtime_error("BruteForceNN: no reference rows");
    Check(mi_icp_feature_match(Engine(), query.data()->data(), (int64_t)query.size(), ref.data()->data(), (int64_t)ref.size(), Dim,
                               indices.data(), distances.data(), nullptr, nullptr));
    Check(mi_icp_synchronize(Engine()));
}
template void BruteForceNN<33>(const utility::device_vector<Eigen::Matrix<float, 33, 1>>&,
                               const utility::device_vector<Eigen::Matrix<float, 33, 1>>&, utility::device_vector<int>&,
                               utility::device_vector<float>&);
template void BruteForceNN<352>(const utility::device_vector<Eigen::Matrix<float, 352, 1>>&,
                                const utility::device_vector<Eigen::Matrix<float, 352, 1>>&, utility::device_vector<int>&,
                                utility::device_vector<float>&);

static void CheckCtx(mi_icp_ctx* c, int rc) {
    if (rc < 0) throw std::runtime_error(std::string("mi_icp: ") + mi_icp_last_error(c));
}

KDTreeFlann::KDTreeFlann() {}
KDTreeFlann::KDTreeFlann(const utility::device_vector<Eigen::Vector3f>& data) { SetRawData(data); }
KDTreeFlann::~KDTreeFlann() {
    if (ctx_) mi_icp_destroy(ctx_);
}

bool KDTreeFlann::SetRawData(const utility::device_vector<Eigen::Vector3f>& data) {
    dataset_size_ = 0;
    if (data.empty()) {
        LogWarning("[KDTreeFlann::SetRawData] Failed due to no data.");   // kdtree_flann.inl:129-132
        return false;
    }
    if (!ctx_) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (mi_icp_create(dev, &ctx_) != MI_ICP_OK)
            throw std::runtime_error("mi_icp_create failed: no MI355X device available (there is no CPU fallback)");
    }
    CheckCtx(ctx_, mi_icp_set_target(ctx_, data.data()->data(), nullptr, nullptr, (int64_t)data.size(), MI_ICP_DEVICE));
    dataset_size_ = data.size();
    return true;
}

int KDTreeFlann::SearchMany(const utility::device_vector<Eigen::Vector3f>& query, int knn, float radius,
                            utility::device_vector<int>& indices, utility::device_vector<float>& distance2) const {
    if (dataset_size_ == 0 || query.empty() || knn <= 0) return -1;   // kdtree_flann.cu:52-54,72-73
    indices.resize(query.size() * (size_t)knn);
    distance2.resize(query.size() * (size_t)knn);
    int64_t found = 0;
    CheckCtx(ctx_, mi_icp_search_knn(ctx_, query.data()->data(), (int64_t)query.size(), knn, radius, indices.data(),
                                     distance2.data(), &found, MI_ICP_DEVICE));
    return (int)found;
}

int KDTreeFlann::SearchKNN(const utility::device_vector<Eigen::Vector3f>& query, int knn,
                           utility::device_vector<int>& indices, utility::device_vector<float>& distance2) const {
    return SearchMany(query, knn, 0.0f, indices, distance2);
}
int KDTreeFlann::SearchRadius(const utility::device_vector<Eigen::Vector3f>& query, float radius, int max_nn,
                              utility::device_vector<int>& indices, utility::device_vector<float>& distance2) const {
    if (radius <= 0.0f) return -1;
    return SearchMany(query, max_nn, radius, indices, distance2);
}
int KDTreeFlann::Search(const utility::device_vector<Eigen::Vector3f>& query, const KDTreeSearchParam& param,
                        utility::device_vector<int>& indices, utility::device_vector<float>& distance2) const {
    switch (param.GetSearchType()) {
        case KDTreeSearchParam::SearchType::Knn:
            return SearchKNN(query, ((const KDTreeSearchParamKNN&)param).knn_, indices, distance2);
        case KDTreeSearchParam::SearchType::Radius:
            return SearchRadius(query, ((const KDTreeSearchParamRadius&)param).radius_,
                                ((const KDTreeSearchParamRadius&)param).max_nn_, indices, distance2);
        default: return -1;
    }
}

// single query: results trimmed to the neighbours found, like FLANN's host overloads
static int One(const KDTreeFlann& tree, const Eigen::Vector3f& query, int knn, float radius, bool is_radius,
               thrust::host_vector<int>& indices, thrust::host_vector<float>& distance2) {
    utility::device_vector<Eigen::Vector3f> q(std::vector<Eigen::Vector3f>{query});
    utility::device_vector<int> di;
    utility::device_vector<float> dd;
    const int k = is_radius ? tree.SearchRadius(q, radius, knn, di, dd) : tree.SearchKNN(q, knn, di, dd);
    indices.clear();
    distance2.clear();
    if (k < 0) return k;
    const auto hi = di.to_host();
    const auto hd = dd.to_host();
    indices.assign(hi.begin(), hi.begin() + k);
    distance2.assign(hd.begin(), hd.begin() + k);
    return k;
}
int KDTreeFlann::SearchKNN(const Eigen::Vector3f& query, int knn, thrust::host_vector<int>& indices,
                           thrust::host_vector<float>& distance2) const {
    return One(*this, query, knn, 0.0f, false, indices, distance2);
}
int KDTreeFlann::SearchRadiusOne(const Eigen::Vector3f& query, float radius, int max_nn,
                                 thrust::host_vector<int>& indices, thrust::host_vector<float>& distance2) const {
    return One(*this, query, max_nn, radius, true, indices, distance2);
}
int KDTreeFlann::Search(const Eigen::Vector3f& query, const KDTreeSearchParam& param, thrust::host_vector<int>& indices,
                        thrust::host_vector<float>& distance2) const {
    switch (param.GetSearchType()) {
        case KDTreeSearchParam::SearchType::Knn:
            return SearchKNN(query, ((const KDTreeSearchParamKNN&)param).knn_, indices, distance2);
        case KDTreeSearchParam::SearchType::Radius:
            return SearchRadiusOne(query, ((const KDTreeSearchParamRadius&)param).radius_,
                                   ((const KDTreeSearchParamRadius&)param).max_nn_, indices, distance2);
        default: return -1;
    }
}

}  // namespace knn

// ---------------------------------------------------------------- odometry
namespace odometry {

static bool OdometryInputsOk(const geometry::RGBDImage& source, const geometry::RGBDImage& target) {
    auto is_float_image = [](const geometry::Image& im) { return im.num_of_channels_ == 1 && im.bytes_per_channel_ == 4; };
    const geometry::Image &sc = source.color_, &sd = source.depth_, &tc = target.color_, &td = target.depth_;
    const bool same = sc.width_ == tc.width_ && sc.height_ == tc.height_ && sd.width_ == td.width_ &&
                      sd.height_ == td.height_ && sc.width_ == sd.width_ && sc.height_ == sd.height_;
    if (same && is_float_image(sc) && is_float_image(sd) && is_float_image(tc) && is_float_image(td)) return true;
    LogWarning("[RGBDOdometry] Two RGBD pairs should be same in size.");  // odometry.cu:845-851
    return false;
}

static mi_icp_odometry_option OdometryOptionC(const OdometryOption& option) {
    mi_icp_odometry_option opt = {};
    opt.num_levels = (int32_t)option.iteration_number_per_pyramid_level_.size();
    for (int i = 0; i < opt.num_levels && i < MI_ICP_ODOMETRY_MAX_LEVELS; ++i)
        opt.iterations[i] = option.iteration_number_per_pyramid_level_[(size_t)i];
    opt.max_depth_diff = option.max_depth_diff_;
    opt.min_depth = option.min_depth_;
    opt.max_depth = option.max_depth_;
    opt.nu = option.nu_;
    opt.sigma2_init = option.sigma2_init_;
    for (int i = 0; i < 6; ++i) opt.inv_sigma_mat_diag[i] = option.inv_sigma_mat_diag_[i];
    return opt;
}

static Eigen::Matrix6f Info6(const double* info) {
    Eigen::Matrix6f I;
    for (int r = 0; r < 6; ++r)
        for (int c2 = 0; c2 < 6; ++c2) I(r, c2) = (float)info[r * 6 + c2];
    return I;
}

std::tuple<bool, Eigen::Matrix4f, Eigen::Matrix6f> ComputeRGBDOdometry(
        const geometry::RGBDImage& source, const geometry::RGBDImage& target,
        const camera::PinholeCameraIntrinsic& intrinsic, const Eigen::Matrix4f& odo_init,
        const RGBDOdometryJacobian& jacobian_method, const OdometryOption& option) {
    if (!OdometryInputsOk(source, target))
        return std::make_tuple(false, Eigen::Matrix4f::Identity(), Eigen::Matrix6f::Zero());
    const mi_icp_odometry_option opt = OdometryOptionC(option);
    const float k4[4] = {intrinsic.fx_, intrinsic.fy_, intrinsic.cx_, intrinsic.cy_};
    int ok = 0;
    Eigen::Matrix4f T;
    double info[36];
    Check(mi_icp_compute_rgbd_odometry(Engine(), (const float*)source.color_.data_.data(),
                                       (const float*)source.depth_.data_.data(),
                                       (const float*)target.color_.data_.data(),
                                       (const float*)target.depth_.data_.data(), source.color_.width_,
                                       source.color_.height_, k4, odo_init.data(), (int)jacobian_method.jacobian_type_,
                                       &opt, &ok, T.data(), info, MI_ICP_DEVICE));
    return std::make_tuple(ok != 0, T, Info6(info));
}

std::tuple<bool, Eigen::Matrix4f, Eigen::Vector6f, Eigen::Matrix6f> ComputeWeightedRGBDOdometry(
        const geometry::RGBDImage& source, const geometry::RGBDImage& target,
        const camera::PinholeCameraIntrinsic& intrinsic, const Eigen::Matrix4f& odo_init,
        const Eigen::Vector6f& prev_twist, const RGBDOdometryJacobian& /*always the hybrid term, odometry.cu:937-941*/,
        const OdometryOption& option) {
    if (!OdometryInputsOk(source, target))
        return std::make_tuple(false, Eigen::Matrix4f::Identity(), Eigen::Vector6f::Zero(), Eigen::Matrix6f::Zero());
    const mi_icp_odometry_option opt = OdometryOptionC(option);
    const float k4[4] = {intrinsic.fx_, intrinsic.fy_, intrinsic.cx_, intrinsic.cy_};
    int ok = 0;
    Eigen::Matrix4f T;
    Eigen::Vector6f twist;
    double info[36];
    Check(mi_icp_compute_weighted_rgbd_odometry(Engine(), (const float*)source.color_.data_.data(),
                                                (const float*)source.depth_.data_.data(),
                                                (const float*)target.color_.data_.data(),
                                                (const float*)target.depth_.data_.data(), source.color_.width_,
                                                source.color_.height_, k4, odo_init.data(), prev_twist.data(), &opt, &ok,
                                                T.data(), twist.data(), info, MI_ICP_DEVICE));
    return std::make_tuple(ok != 0, T, twist, Info6(info));
}

}  // namespace odometry

// ---------------------------------------------------------------- occupancy grid
namespace geometry {

namespace {
mi_icp_occgrid_params OccParams(const OccupancyGrid& g) {
    mi_icp_occgrid_params p;
    p.voxel_size = g.voxel_size_;
    for (int k = 0; k < 3; ++k) p.origin[k] = g.origin_[k];
    p.clamping_thres_min = g.clamping_thres_min_;
    p.clamping_thres_max = g.clamping_thres_max_;
    p.prob_hit_log = g.prob_hit_log_;
    p.prob_miss_log = g.prob_miss_log_;
    p.occ_prob_thres_log = g.occ_prob_thres_log_;
    return p;
}
}  // namespace

OccupancyGrid::OccupancyGrid() : OccupancyGrid(0.05f, 512, Eigen::Vector3f::Zero()) {}

OccupancyGrid::OccupancyGrid(float voxel_size, size_t resolution, const Eigen::Vector3f& origin)
    : GeometryBase3D(GeometryType::OccupancyGrid), voxel_size_(voxel_size), resolution_((int)resolution), origin_(origin) {
    min_bound_ = max_bound_ = Eigen::Vector3i(resolution_ / 2, resolution_ / 2, resolution_ / 2);
}

OccupancyGrid::~OccupancyGrid() {
    if (grid_) (void)mi_icp_occgrid_destroy(Engine(), grid_);
}

mi_icp_occgrid* OccupancyGrid::Handle() const {
    if (!grid_) {
        Check(mi_icp_occgrid_create(Engine(), resolution_, &grid_));
        made_resolution_ = resolution_;
        RefreshBounds();
    } else if (made_resolution_ != resolution_) {
        const int rc = mi_icp_occgrid_reconstruct(Engine(), grid_, resolution_);
        if (rc == MI_ICP_ERR_HIP) grid_ = nullptr;  // (the planes could not be made: the handle is gone)
        Check(rc);
        made_resolution_ = resolution_;
        RefreshBounds();
    }
    return grid_;
}

void OccupancyGrid::RefreshBounds() const {
    Check(mi_icp_occgrid_get_bounds(Engine(), grid_, min_bound_.data(), max_bound_.data()));
}

OccupancyGrid& OccupancyGrid::Clear() {
    if (grid_ && made_resolution_ == resolution_) Check(mi_icp_occgrid_reset(Engine(), grid_));
    min_bound_ = max_bound_ = Eigen::Vector3i(resolution_ / 2, resolution_ / 2, resolution_ / 2);
    return *this;
}

Eigen::Vector3f OccupancyGrid::GetMinBound() const {
    const int h = resolution_ / 2;
    Eigen::Vector3f out;
    for (int k = 0; k < 3; ++k) out[k] = (float)(min_bound_[k] - h) * voxel_size_ + origin_[k];
    return out;
}

Eigen::Vector3f OccupancyGrid::GetMaxBound() const {
    const int h = resolution_ / 2;
    Eigen::Vector3f out;
    for (int k = 0; k < 3; ++k) out[k] = (float)(max_bound_[k] - (h - 1)) * voxel_size_ + origin_[k];
    return out;
}

AxisAlignedBoundingBox3 OccupancyGrid::GetAxisAlignedBoundingBox() const {
    return AxisAlignedBoundingBox3(GetMinBound(), GetMaxBound());
}

OccupancyGrid& OccupancyGrid::Transform(const Eigen::Matrix4f&) {
    LogError("OccupancyGrid::Transform is not supported");
    return *this;
}

OccupancyGrid& OccupancyGrid::Rotate(const Eigen::Matrix3f&, bool) {
    LogError("OccupancyGrid::Rotate is not supported");
    return *this;
}

OccupancyGrid& OccupancyGrid::Translate(const Eigen::Vector3f& translation, bool relative) {
    origin_ = relative ? origin_ + translation : translation;
    return *this;
}

OccupancyGrid& OccupancyGrid::Scale(const float scale, bool) {
    voxel_size_ *= scale;
    return *this;
}

utility::device_vector<float> OccupancyGrid::GetProbLog(const utility::device_vector<Eigen::Vector3f>& points) const {
    utility::device_vector<float> out(points.size());
    if (points.empty()) return out;
    const mi_icp_occgrid_params p = OccParams(*this);
    Check(mi_icp_occgrid_query(Engine(), Handle(), &p, Ptr(points), (int64_t)points.size(), out.data(), nullptr));
    Check(mi_icp_synchronize(Engine()));
    return out;
}

std::tuple<bool, OccupancyVoxel> OccupancyGrid::GetVoxel(const Eigen::Vector3f& point) const {
    const mi_icp_occgrid_params p = OccParams(*this);
    utility::device_vector<Eigen::Vector3f> pt(std::vector<Eigen::Vector3f>{point});
    utility::device_vector<float> prob(1);
    utility::device_vector<Eigen::Vector3i> idx(1);
    Check(mi_icp_occgrid_query(Engine(), Handle(), &p, Ptr(pt), 1, prob.data(), idx.data()->data()));
    Check(mi_icp_synchronize(Engine()));
    const float v = prob.to_host()[0];
    if (std::isnan(v)) return std::make_tuple(false, OccupancyVoxel());
    return std::make_tuple(true, OccupancyVoxel(idx.to_host()[0], v));
}

bool OccupancyGrid::IsOccupied(const Eigen::Vector3f& point) const {
    const auto r = GetVoxel(point);
    return std::get<0>(r) && std::get<1>(r).prob_log_ > occ_prob_thres_log_;
}

bool OccupancyGrid::IsUnknown(const Eigen::Vector3f& point) const { return !std::get<0>(GetVoxel(point)); }

std::shared_ptr<std::vector<OccupancyVoxel>> OccupancyGrid::Extract(int which) const {
    const mi_icp_occgrid_params p = OccParams(*this);
    mi_icp_occgrid* g = Handle();
    auto out = std::make_shared<std::vector<OccupancyVoxel>>();
    int64_t m = 0;
    Check(mi_icp_occgrid_extract(Engine(), g, &p, which, nullptr, nullptr, nullptr, 0, &m));
    if (m == 0) return out;
    utility::device_vector<Eigen::Vector3i> idx((size_t)m);
    utility::device_vector<float> prob((size_t)m);
    Check(mi_icp_occgrid_extract(Engine(), g, &p, which, idx.data()->data(), prob.data(), nullptr, m, &m));
    Check(mi_icp_synchronize(Engine()));
    const std::vector<Eigen::Vector3i> hi = idx.to_host();
    const std::vector<float> hp = prob.to_host();
    out->reserve((size_t)m);
    for (size_t i = 0; i < (size_t)m; ++i) out->push_back(OccupancyVoxel(hi[i], hp[i]));
    return out;
}

std::shared_ptr<std::vector<OccupancyVoxel>> OccupancyGrid::ExtractKnownVoxels() const { return Extract(MI_ICP_OCCGRID_KNOWN); }
std::shared_ptr<std::vector<OccupancyVoxel>> OccupancyGrid::ExtractFreeVoxels() const { return Extract(MI_ICP_OCCGRID_FREE); }
std::shared_ptr<std::vector<OccupancyVoxel>> OccupancyGrid::ExtractOccupiedVoxels() const { return Extract(MI_ICP_OCCGRID_OCCUPIED); }

OccupancyGrid& OccupancyGrid::Reconstruct(float voxel_size, int resolution) {
    voxel_size_ = voxel_size;
    resolution_ = resolution;
    if (grid_) {
        made_resolution_ = 0;  // (also for the same resolution: every voxel unknown again)
        (void)Handle();
    } else {
        min_bound_ = max_bound_ = Eigen::Vector3i(resolution_ / 2, resolution_ / 2, resolution_ / 2);
    }
    return *this;
}

OccupancyGrid& OccupancyGrid::SetFreeArea(const Eigen::Vector3f& min_bound, const Eigen::Vector3f& max_bound) {
    const mi_icp_occgrid_params p = OccParams(*this);
    Check(mi_icp_occgrid_set_free_area(Engine(), Handle(), &p, min_bound.data(), max_bound.data()));
    RefreshBounds();
    return *this;
}

OccupancyGrid& OccupancyGrid::Insert(const utility::device_vector<Eigen::Vector3f>& points, const Eigen::Vector3f& viewpoint,
                                     float max_range) {
    if (points.empty()) return *this;
    const mi_icp_occgrid_params p = OccParams(*this);
    Check(mi_icp_occgrid_insert(Engine(), Handle(), &p, Ptr(points), (int64_t)points.size(), viewpoint.data(), max_range));
    RefreshBounds();
    return *this;
}

OccupancyGrid& OccupancyGrid::Insert(const thrust::host_vector<Eigen::Vector3f>& points, const Eigen::Vector3f& viewpoint,
                                     float max_range) {
    return Insert(utility::device_vector<Eigen::Vector3f>(points), viewpoint, max_range);
}

OccupancyGrid& OccupancyGrid::Insert(const PointCloud& pointcloud, const Eigen::Vector3f& viewpoint, float max_range) {
    return Insert(pointcloud.points_, viewpoint, max_range);
}

OccupancyGrid& OccupancyGrid::AddVoxel(const Eigen::Vector3i& voxel, bool occupied) {
    return AddVoxels(utility::device_vector<Eigen::Vector3i>(std::vector<Eigen::Vector3i>{voxel}), occupied);
}

OccupancyGrid& OccupancyGrid::AddVoxels(const utility::device_vector<Eigen::Vector3i>& voxels, bool occupied) {
    if (voxels.empty()) return *this;
    const mi_icp_occgrid_params p = OccParams(*this);
    mi_icp_occgrid* g = Handle();
    const int rc = mi_icp_occgrid_add_voxels(Engine(), g, &p, voxels.data()->data(), (int64_t)voxels.size(), occupied ? 1 : 0);
    if (rc == MI_ICP_ERR_INVALID) {  // an index outside the grid: logged, nothing changed (occupancygrid.cu:551-555)
        LogError(mi_icp_last_error(Engine()));
        return *this;
    }
    Check(rc);
    RefreshBounds();
    return *this;
}

std::vector<float> OccupancyGrid::GetVoxels() const {
    const size_t n = (size_t)resolution_ * (size_t)resolution_ * (size_t)resolution_;
    mi_icp_occgrid* g = Handle();
    utility::device_vector<float> plane(n);
    Check(mi_icp_occgrid_get_voxels(Engine(), g, plane.data()));
    return plane.to_host();
}

std::shared_ptr<PointCloud> PointCloud::CreateFromOccupancyGrid(const OccupancyGrid& occgrid) {
    auto out = std::make_shared<PointCloud>();
    const mi_icp_occgrid_params p = OccParams(occgrid);
    mi_icp_occgrid* g = occgrid.Handle();
    int64_t m = 0;
    Check(mi_icp_occgrid_extract(Engine(), g, &p, MI_ICP_OCCGRID_OCCUPIED, nullptr, nullptr, nullptr, 0, &m));
    if (m == 0) return out;
    out->points_.resize((size_t)m);
    Check(mi_icp_occgrid_extract(Engine(), g, &p, MI_ICP_OCCGRID_OCCUPIED, nullptr, nullptr, out->points_.data()->data(), m, &m));
    Check(mi_icp_synchronize(Engine()));
    out->colors_ = std::vector<Eigen::Vector3f>((size_t)m, Eigen::Vector3f(0.0f, 0.0f, 1.0f));
    return out;
}

// ---- geometry::VoxelGrid (geometry/voxelgrid.cu, voxelgrid_factory.cu) over mi_icp_voxelgrid_*
namespace {

void Copy2D(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    if (rows == 0) return;
    const hipError_t e = hipMemcpy2D(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) throw std::runtime_error(std::string("hipMemcpy2D: ") + hipGetErrorString(e));
}

// the colours of voxels_values_ as the packed array the engine takes
utility::device_vector<Eigen::Vector3f> VoxelColors(const utility::device_vector<Voxel>& values) {
    utility::device_vector<Eigen::Vector3f> c(values.size());
    Copy2D(c.data(), sizeof(Eigen::Vector3f), (const char*)values.data() + offsetof(Voxel, color_), sizeof(Voxel),
           sizeof(Eigen::Vector3f), values.size());
    return c;
}

// ... and the way back: the first m keys and colours become the grid's voxels
void SetVoxelArrays(VoxelGrid* g, utility::device_vector<Eigen::Vector3i>& keys, const utility::device_vector<Eigen::Vector3f>& colors,
                    size_t m) {
    keys.resize(m);
    g->voxels_values_ = utility::device_vector<Voxel>(m);
    Copy2D((char*)g->voxels_values_.data() + offsetof(Voxel, grid_index_), sizeof(Voxel), keys.data(), sizeof(Eigen::Vector3i),
           sizeof(Eigen::Vector3i), m);
    Copy2D((char*)g->voxels_values_.data() + offsetof(Voxel, color_), sizeof(Voxel), colors.data(), sizeof(Eigen::Vector3f),
           sizeof(Eigen::Vector3f), m);
    g->voxels_keys_.swap(keys);
}

const int32_t* KeyPtr(const utility::device_vector<Eigen::Vector3i>& v) { return v.empty() ? nullptr : v.data()->data(); }
int32_t* KeyPtr(utility::device_vector<Eigen::Vector3i>& v) { return v.empty() ? nullptr : v.data()->data(); }
float* ColPtr(utility::device_vector<Eigen::Vector3f>& v) { return v.empty() ? nullptr : v.data()->data(); }

// a refusal of the engine is what the reference logs as an error
bool Refused(int rc) {
    if (rc == MI_ICP_ERR_INVALID) {
        LogError(mi_icp_last_error(Engine()));
        return true;
    }
    Check(rc);
    return false;
}

int FloorIndex(float x) { return (int)std::fmin(std::fmax(std::floor(x), -1.0e9f), 1.0e9f); }

int RoundCount(float extent, float voxel_size) { return (int)std::round(extent / voxel_size); }

}  // namespace

VoxelGrid::VoxelGrid() : GeometryBase3D(GeometryType::VoxelGrid) {}
VoxelGrid::~VoxelGrid() {}
VoxelGrid::VoxelGrid(const VoxelGrid& o)
    : GeometryBase3D(GeometryType::VoxelGrid),
      voxel_size_(o.voxel_size_),
      origin_(o.origin_),
      voxels_keys_(o.voxels_keys_),
      voxels_values_(o.voxels_values_),
      sorted_(o.sorted_) {}

std::pair<thrust::host_vector<Eigen::Vector3i>, thrust::host_vector<Voxel>> VoxelGrid::GetVoxels() const {
    return std::make_pair(voxels_keys_.to_host(), voxels_values_.to_host());
}

void VoxelGrid::SetVoxels(const thrust::host_vector<Eigen::Vector3i>& voxels_keys, const thrust::host_vector<Voxel>& voxels_values) {
    voxels_keys_ = voxels_keys;
    voxels_values_ = voxels_values;
    sorted_ = false;
}

VoxelGrid& VoxelGrid::Clear() {
    voxel_size_ = 0.0f;
    origin_ = Eigen::Vector3f::Zero();
    voxels_keys_.clear();
    voxels_values_.clear();
    sorted_ = true;
    return *this;
}

bool VoxelGrid::IsEmpty() const { return voxels_keys_.empty(); }

namespace {
struct IndexBounds {
    Eigen::Vector3i lo, hi;
    double sum[3];
};
IndexBounds GetIndexBounds(const VoxelGrid& g) {
    IndexBounds b;
    Check(mi_icp_voxelgrid_bounds(Engine(), KeyPtr(g.voxels_keys_), (int64_t)g.voxels_keys_.size(), g.voxel_size_, g.origin_.data(),
                                  b.lo.data(), b.hi.data(), b.sum));
    return b;
}
}  // namespace

Eigen::Vector3f VoxelGrid::GetMinBound() const {
    if (voxels_keys_.empty()) return origin_;
    const IndexBounds b = GetIndexBounds(*this);
    Eigen::Vector3f out;
    for (int k = 0; k < 3; ++k) out[k] = (float)b.lo[k] * voxel_size_ + origin_[k];
    return out;
}

Eigen::Vector3f VoxelGrid::GetMaxBound() const {
    if (voxels_keys_.empty()) return origin_;
    const IndexBounds b = GetIndexBounds(*this);
    Eigen::Vector3f out;
    for (int k = 0; k < 3; ++k) out[k] = ((float)b.hi[k] + 1.0f) * voxel_size_ + origin_[k];
    return out;
}

Eigen::Vector3f VoxelGrid::GetCenter() const {
    Eigen::Vector3f out = Eigen::Vector3f::Zero();
    if (voxels_keys_.empty()) return out;
    const IndexBounds b = GetIndexBounds(*this);
    for (int k = 0; k < 3; ++k) out[k] = (float)(b.sum[k] / (double)voxels_keys_.size());
    return out;
}

AxisAlignedBoundingBox3 VoxelGrid::GetAxisAlignedBoundingBox() const {
    return AxisAlignedBoundingBox3(GetMinBound(), GetMaxBound());
}

VoxelGrid& VoxelGrid::Transform(const Eigen::Matrix4f&) {
    LogError("VoxelGrid::Transform is not supported");
    return *this;
}

VoxelGrid& VoxelGrid::Rotate(const Eigen::Matrix3f&, bool) {
    LogError("VoxelGrid::Rotate is not supported");
    return *this;
}

VoxelGrid& VoxelGrid::Translate(const Eigen::Vector3f& translation, bool) {
    origin_ += translation;
    return *this;
}

VoxelGrid& VoxelGrid::Scale(const float scale, bool) {
    voxel_size_ *= scale;
    return *this;
}

namespace {
// this grid's voxels, then `keys` / `colors`: one voxel per key, ascending (include/mi_icp.h, merge)
void MergeInto(VoxelGrid* g, const utility::device_vector<Eigen::Vector3i>& keys, utility::device_vector<Eigen::Vector3f>& colors,
               int mode) {
    utility::device_vector<Eigen::Vector3f> mine = VoxelColors(g->voxels_values_);
    const size_t cap = g->voxels_keys_.size() + keys.size();
    utility::device_vector<Eigen::Vector3i> ok(cap);
    utility::device_vector<Eigen::Vector3f> oc(cap);
    int64_t m = 0;
    Check(mi_icp_voxelgrid_merge(Engine(), KeyPtr(g->voxels_keys_), ColPtr(mine), (int64_t)g->voxels_keys_.size(), KeyPtr(keys),
                                 ColPtr(colors), (int64_t)keys.size(), mode, KeyPtr(ok), ColPtr(oc), (int64_t)cap, &m));
    SetVoxelArrays(g, ok, oc, (size_t)m);
}

void KeysOfVoxels(const utility::device_vector<Voxel>& voxels, utility::device_vector<Eigen::Vector3i>* keys) {
    keys->resize(voxels.size());
    Copy2D(keys->data(), sizeof(Eigen::Vector3i), (const char*)voxels.data() + offsetof(Voxel, grid_index_), sizeof(Voxel),
           sizeof(Eigen::Vector3i), voxels.size());
}
}  // namespace

VoxelGrid& VoxelGrid::operator+=(const VoxelGrid& voxelgrid) {
    char msg[256];
    if (voxel_size_ != voxelgrid.voxel_size_) {
        std::snprintf(msg, sizeof(msg), "[VoxelGrid] Could not combine VoxelGrid because voxel_size differs (this=%f, other=%f)",
                      voxel_size_, voxelgrid.voxel_size_);
        LogError(msg);
    }
    if (!(origin_ == voxelgrid.origin_)) {
        std::snprintf(msg, sizeof(msg), "[VoxelGrid] Could not combine VoxelGrid because origin differs (this=%f,%f,%f, other=%f,%f,%f)",
                      origin_(0), origin_(1), origin_(2), voxelgrid.origin_(0), voxelgrid.origin_(1), voxelgrid.origin_(2));
        LogError(msg);
    }
    utility::device_vector<Eigen::Vector3f> theirs = VoxelColors(voxelgrid.voxels_values_);
    MergeInto(this, voxelgrid.voxels_keys_, theirs, MI_ICP_VOXELGRID_AVERAGE);
    sorted_ = true;
    return *this;
}

VoxelGrid VoxelGrid::operator+(const VoxelGrid& voxelgrid) const { return (VoxelGrid(*this) += voxelgrid); }

Eigen::Vector3i VoxelGrid::GetVoxel(const Eigen::Vector3f& point) const {
    Eigen::Vector3i out;
    for (int k = 0; k < 3; ++k) out[k] = FloorIndex((point[k] - origin_[k]) / voxel_size_);
    return out;
}

Eigen::Vector3f VoxelGrid::GetVoxelCenterCoordinate(const Eigen::Vector3i& idx) const {
    // the reference's thrust::find, on the host: one key is looked up, not a batch
    const std::vector<Eigen::Vector3i> keys = voxels_keys_.to_host();
    for (const Eigen::Vector3i& k : keys) {
        if (k == idx) {
            Eigen::Vector3f out;
            for (int d = 0; d < 3; ++d) out[d] = ((float)idx[d] + 0.5f) * voxel_size_ + origin_[d];
            return out;
        }
    }
    return Eigen::Vector3f::Zero();
}

std::array<Eigen::Vector3f, 8> VoxelGrid::GetVoxelBoundingPoints(const Eigen::Vector3i& index) const {
    const float r = voxel_size_ / 2.0f;
    const Eigen::Vector3f x = GetVoxelCenterCoordinate(index);
    std::array<Eigen::Vector3f, 8> p;
    p[0] = x + Eigen::Vector3f(-r, -r, -r);
    p[1] = x + Eigen::Vector3f(-r, -r, r);
    p[2] = x + Eigen::Vector3f(r, -r, -r);
    p[3] = x + Eigen::Vector3f(r, -r, r);
    p[4] = x + Eigen::Vector3f(-r, r, -r);
    p[5] = x + Eigen::Vector3f(-r, r, r);
    p[6] = x + Eigen::Vector3f(r, r, -r);
    p[7] = x + Eigen::Vector3f(r, r, r);
    return p;
}

void VoxelGrid::AddVoxel(const Voxel& voxel) { AddVoxels(std::vector<Voxel>{voxel}); }

void VoxelGrid::AddVoxels(const utility::device_vector<Voxel>& voxels) {
    if (voxels.empty()) return;
    utility::device_vector<Eigen::Vector3i> keys;
    KeysOfVoxels(voxels, &keys);
    utility::device_vector<Eigen::Vector3f> colors = VoxelColors(voxels);
    MergeInto(this, keys, colors, MI_ICP_VOXELGRID_KEEP_FIRST);
    sorted_ = true;
}

void VoxelGrid::AddVoxels(const thrust::host_vector<Voxel>& voxels) { AddVoxels(utility::device_vector<Voxel>(voxels)); }

VoxelGrid& VoxelGrid::PaintUniformColor(const Eigen::Vector3f& color) {
    const size_t m = voxels_values_.size();
    if (m == 0) return *this;
    utility::device_vector<Eigen::Vector3f> c(m);
    Check(mi_icp_voxelgrid_paint(Engine(), ColPtr(c), (int64_t)m, nullptr, 0, color.data()));
    Copy2D((char*)voxels_values_.data() + offsetof(Voxel, color_), sizeof(Voxel), c.data(), sizeof(Eigen::Vector3f), sizeof(Eigen::Vector3f), m);
    return *this;
}

VoxelGrid& VoxelGrid::PaintIndexedColor(const utility::device_vector<size_t>& indices, const Eigen::Vector3f& color) {
    const size_t m = voxels_values_.size();
    if (indices.empty()) return *this;
    utility::device_vector<Eigen::Vector3f> c = VoxelColors(voxels_values_);
    if (Refused(mi_icp_voxelgrid_paint(Engine(), ColPtr(c), (int64_t)m, (const int64_t*)indices.data(), (int64_t)indices.size(), color.data())))
        return *this;
    Copy2D((char*)voxels_values_.data() + offsetof(Voxel, color_), sizeof(Voxel), c.data(), sizeof(Eigen::Vector3f), sizeof(Eigen::Vector3f), m);
    return *this;
}

thrust::host_vector<bool> VoxelGrid::CheckIfIncluded(const thrust::host_vector<Eigen::Vector3f>& queries) {
    thrust::host_vector<bool> output(queries.size(), false);
    if (queries.empty()) return output;
    const utility::device_vector<Eigen::Vector3f> q(queries);
    utility::device_vector<uint8_t> inc(queries.size());
    if (Refused(mi_icp_voxelgrid_query(Engine(), KeyPtr(voxels_keys_), (int64_t)voxels_keys_.size(), sorted_ ? 1 : 0, voxel_size_,
                                       origin_.data(), Ptr(q), (int64_t)q.size(), inc.data(), nullptr)))
        return output;
    const std::vector<uint8_t> h = inc.to_host();
    for (size_t i = 0; i < h.size(); ++i) output[i] = h[i] != 0;
    return output;
}

namespace {
VoxelGrid& Carve(VoxelGrid* g, const Image& image, const camera::PinholeCameraParameters& cam, bool keep, const char* what) {
    if (image.height_ != cam.intrinsic_.height_ || image.width_ != cam.intrinsic_.width_) {
        LogError((std::string("[VoxelGrid] provided ") + what + " dimensions are not compatible with the provided camera_parameters").c_str());
        return *g;
    }
    const size_t m = g->voxels_keys_.size();
    if (m == 0) return *g;
    utility::device_vector<Eigen::Vector3f> colors = VoxelColors(g->voxels_values_);
    utility::device_vector<Eigen::Vector3i> ok(m);
    utility::device_vector<Eigen::Vector3f> oc(m);
    const float intr[4] = {cam.intrinsic_.fx_, cam.intrinsic_.fy_, cam.intrinsic_.cx_, cam.intrinsic_.cy_};
    int64_t mo = 0;
    if (Refused(mi_icp_voxelgrid_carve(Engine(), KeyPtr(g->voxels_keys_), ColPtr(colors), (int64_t)m, g->voxel_size_, g->origin_.data(),
                                       image.data_.data(), image.width_, image.height_, image.num_of_channels_,
                                       image.bytes_per_channel_, intr, cam.extrinsic_.data(), keep ? 1 : 0, KeyPtr(ok), ColPtr(oc), &mo)))
        return *g;
    SetVoxelArrays(g, ok, oc, (size_t)mo);
    return *g;
}
}  // namespace

VoxelGrid& VoxelGrid::CarveDepthMap(const Image& depth_map, const camera::PinholeCameraParameters& camera_parameter,
                                    bool keep_voxels_outside_image) {
    return Carve(this, depth_map, camera_parameter, keep_voxels_outside_image, "depth_map");
}

VoxelGrid& VoxelGrid::CarveSilhouette(const Image& silhouette_mask, const camera::PinholeCameraParameters& camera_parameter,
                                      bool keep_voxels_outside_image) {
    return Carve(this, silhouette_mask, camera_parameter, keep_voxels_outside_image, "silhouette_mask");
}

std::shared_ptr<VoxelGrid> VoxelGrid::SelectByIndex(const utility::device_vector<size_t>& indices, bool invert) {
    auto dst = std::make_shared<VoxelGrid>();
    dst->voxel_size_ = voxel_size_;
    dst->origin_ = origin_;
    const size_t m = voxels_keys_.size(), rows = invert ? m : indices.size();
    utility::device_vector<Eigen::Vector3f> colors = VoxelColors(voxels_values_);
    utility::device_vector<Eigen::Vector3i> ok(rows);
    utility::device_vector<Eigen::Vector3f> oc(rows);
    int64_t mo = 0;
    if (Refused(mi_icp_voxelgrid_select_by_index(Engine(), KeyPtr(voxels_keys_), ColPtr(colors), (int64_t)m,
                                                 indices.empty() ? nullptr : (const int64_t*)indices.data(), (int64_t)indices.size(),
                                                 invert ? 1 : 0, KeyPtr(ok), ColPtr(oc), &mo)))
        return dst;
    SetVoxelArrays(dst.get(), ok, oc, (size_t)mo);
    dst->sorted_ = false;
    return dst;
}

std::shared_ptr<VoxelGrid> VoxelGrid::CreateDense(const Eigen::Vector3f& origin, float voxel_size, float width, float height, float depth) {
    auto output = std::make_shared<VoxelGrid>();
    output->origin_ = origin;
    output->voxel_size_ = voxel_size;
    const int nw = RoundCount(width, voxel_size), nh = RoundCount(height, voxel_size), nd = RoundCount(depth, voxel_size);
    int64_t m = 0;
    if (Refused(mi_icp_voxelgrid_dense(Engine(), nw, nh, nd, nullptr, nullptr, 0, &m)) || m == 0) return output;
    utility::device_vector<Eigen::Vector3i> ok((size_t)m);
    utility::device_vector<Eigen::Vector3f> oc((size_t)m);
    Check(mi_icp_voxelgrid_dense(Engine(), nw, nh, nd, KeyPtr(ok), ColPtr(oc), m, &m));
    SetVoxelArrays(output.get(), ok, oc, (size_t)m);
    return output;
}

std::shared_ptr<VoxelGrid> VoxelGrid::CreateFromPointCloudWithinBounds(const PointCloud& input, float voxel_size,
                                                                      const Eigen::Vector3f& min_bound, const Eigen::Vector3f& max_bound) {
    auto output = std::make_shared<VoxelGrid>();
    output->voxel_size_ = voxel_size;
    output->origin_ = min_bound;
    const size_t n = input.points_.size();
    utility::device_vector<Eigen::Vector3i> ok(n);
    utility::device_vector<Eigen::Vector3f> oc(n);
    int64_t m = 0;
    if (Refused(mi_icp_voxelgrid_from_points(Engine(), Ptr(input.points_), input.HasColors() ? Ptr(input.colors_) : nullptr, (int64_t)n,
                                             voxel_size, min_bound.data(), max_bound.data(), KeyPtr(ok), ColPtr(oc), (int64_t)n, &m)))
        return output;
    SetVoxelArrays(output.get(), ok, oc, (size_t)m);
    return output;
}

std::shared_ptr<VoxelGrid> VoxelGrid::CreateFromPointCloud(const PointCloud& input, float voxel_size) {
    const Eigen::Vector3f half = Eigen::Vector3f(voxel_size, voxel_size, voxel_size) * 0.5f;
    return CreateFromPointCloudWithinBounds(input, voxel_size, input.GetMinBound() - half, input.GetMaxBound() + half);
}

std::shared_ptr<VoxelGrid> VoxelGrid::CreateFromOccupancyGrid(const OccupancyGrid& input) {
    auto output = std::make_shared<VoxelGrid>();
    if (input.voxel_size_ <= 0.0f) {
        LogError("[CreateFromOccupancyGrid] occupancy grid  voxel_size <= 0.");
        return output;
    }
    output->voxel_size_ = input.voxel_size_;
    output->origin_ = input.origin_;
    const mi_icp_occgrid_params p = OccParams(input);
    mi_icp_occgrid* g = input.Handle();
    int64_t m = 0;
    Check(mi_icp_occgrid_extract(Engine(), g, &p, MI_ICP_OCCGRID_OCCUPIED, nullptr, nullptr, nullptr, 0, &m));
    if (m == 0) return output;
    utility::device_vector<Eigen::Vector3i> ok((size_t)m);
    utility::device_vector<Eigen::Vector3f> oc((size_t)m);
    Check(mi_icp_occgrid_extract(Engine(), g, &p, MI_ICP_OCCGRID_OCCUPIED, KeyPtr(ok), nullptr, nullptr, m, &m));
    const float blue[3] = {0.0f, 0.0f, 1.0f};
    Check(mi_icp_voxelgrid_paint(Engine(), ColPtr(oc), m, nullptr, 0, blue));
    SetVoxelArrays(output.get(), ok, oc, (size_t)m);
    return output;
}

// ---- geometry::LineSet<3> (lineset.cu): the cloud's bounds and moves on its points
LineSet<3>::LineSet() : GeometryBase3D(GeometryType::LineSet) {}
LineSet<3>::LineSet(const utility::device_vector<Eigen::Vector3f>& points, const utility::device_vector<Eigen::Vector2i>& lines)
    : GeometryBase3D(GeometryType::LineSet), points_(points), lines_(lines) {}
LineSet<3>::LineSet(const thrust::host_vector<Eigen::Vector3f>& points, const thrust::host_vector<Eigen::Vector2i>& lines)
    : GeometryBase3D(GeometryType::LineSet), points_(points), lines_(lines) {}
LineSet<3>::~LineSet() {}

LineSet<3>& LineSet<3>::Clear() {
    points_.clear();
    lines_.clear();
    colors_.clear();
    return *this;
}
Eigen::Vector3f LineSet<3>::GetMinBound() const {
    Eigen::Vector3f b;
    Bounds(points_, &b, nullptr, nullptr);
    return b;
}
Eigen::Vector3f LineSet<3>::GetMaxBound() const {
    Eigen::Vector3f b;
    Bounds(points_, nullptr, &b, nullptr);
    return b;
}
Eigen::Vector3f LineSet<3>::GetCenter() const {
    Eigen::Vector3f b;
    Bounds(points_, nullptr, nullptr, &b);
    return b;
}
AxisAlignedBoundingBox3 LineSet<3>::GetAxisAlignedBoundingBox() const {
    Eigen::Vector3f mn, mx;
    Bounds(points_, &mn, &mx, nullptr);
    return AxisAlignedBoundingBox3(mn, mx);
}
LineSet<3>& LineSet<3>::Transform(const Eigen::Matrix4f& transformation) {
    Check(mi_icp_transform(Engine(), transformation.data(), points_.empty() ? nullptr : points_.data()->data(), nullptr, nullptr,
                           (int64_t)points_.size(), MI_ICP_DEVICE));
    return *this;
}
LineSet<3>& LineSet<3>::Translate(const Eigen::Vector3f& translation, bool relative) {
    Eigen::Vector3f t = translation;
    if (!relative) t -= GetCenter();
    Check(mi_icp_affine(Engine(), nullptr, 0.0f, 0, nullptr, t.data(), points_.empty() ? nullptr : points_.data()->data(), nullptr, nullptr,
                        (int64_t)points_.size(), MI_ICP_DEVICE));
    return *this;
}
LineSet<3>& LineSet<3>::Scale(const float scale, bool center) {
    Eigen::Vector3f c = Eigen::Vector3f::Zero();
    const bool use_c = center && !points_.empty();
    if (use_c) c = GetCenter();
    Check(mi_icp_affine(Engine(), nullptr, scale, 1, use_c ? c.data() : nullptr, nullptr, points_.empty() ? nullptr : points_.data()->data(),
                        nullptr, nullptr, (int64_t)points_.size(), MI_ICP_DEVICE));
    return *this;
}
LineSet<3>& LineSet<3>::Rotate(const Eigen::Matrix3f& R, bool center) {
    Eigen::Vector3f c = Eigen::Vector3f::Zero();
    const bool use_c = center && !points_.empty();
    if (use_c) c = GetCenter();
    Check(mi_icp_affine(Engine(), R.data(), 0.0f, 0, use_c ? c.data() : nullptr, nullptr, points_.empty() ? nullptr : points_.data()->data(),
                        nullptr, nullptr, (int64_t)points_.size(), MI_ICP_DEVICE));
    return *this;
}
std::pair<Eigen::Vector3f, Eigen::Vector3f> LineSet<3>::GetLineCoordinate(size_t line_index) const {
    std::pair<Eigen::Vector3f, Eigen::Vector3f> out(Eigen::Vector3f::Zero(), Eigen::Vector3f::Zero());
    if (line_index >= lines_.size()) return out;
    Eigen::Vector2i l;
    utility::hip_check(hipMemcpy(&l, lines_.data() + line_index, sizeof(l), hipMemcpyDeviceToHost), "hipMemcpy");
    if (l(0) < 0 || l(1) < 0 || (size_t)l(0) >= points_.size() || (size_t)l(1) >= points_.size()) return out;
    utility::hip_check(hipMemcpy(&out.first, points_.data() + l(0), sizeof(Eigen::Vector3f), hipMemcpyDeviceToHost), "hipMemcpy");
    utility::hip_check(hipMemcpy(&out.second, points_.data() + l(1), sizeof(Eigen::Vector3f), hipMemcpyDeviceToHost), "hipMemcpy");
    return out;
}
LineSet<3>& LineSet<3>::PaintUniformColor(const Eigen::Vector3f& color) {
    colors_ = std::vector<Eigen::Vector3f>(lines_.size(), color);
    return *this;
}
std::shared_ptr<LineSet<3>> LineSet<3>::CreateFromAxisAlignedBoundingBox(const AxisAlignedBoundingBox3& box) {
    const Eigen::Vector3f lo = box.GetMinBound(), hi = box.GetMaxBound();
    std::vector<Eigen::Vector3f> p = {{lo(0), lo(1), lo(2)}, {hi(0), lo(1), lo(2)}, {hi(0), hi(1), lo(2)}, {lo(0), hi(1), lo(2)},
                                      {lo(0), lo(1), hi(2)}, {hi(0), lo(1), hi(2)}, {hi(0), hi(1), hi(2)}, {lo(0), hi(1), hi(2)}};
    const int e[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
    std::vector<Eigen::Vector2i> l;
    for (auto& q : e) {
        Eigen::Vector2i v;
        v(0) = q[0];
        v(1) = q[1];
        l.push_back(v);
    }
    return std::make_shared<LineSet<3>>(p, l);
}

// ---- geometry::DistanceTransform (distancetransform.cu, distancetransform_factory.cu, densegrid.inl) over mi_icp_dt_*
namespace {
DistanceVoxel MakeDistanceVoxel(const Eigen::Vector3i& nearest, float distance) {
    DistanceVoxel v;
    v.nearest_index_ = Eigen::Vector3ui16((unsigned short)nearest[0], (unsigned short)nearest[1], (unsigned short)nearest[2]);
    v.state_ = nearest[0] < 0 ? (unsigned char)DistanceVoxel::NotSite : (unsigned char)0;
    v.distance_ = distance;
    return v;
}
}  // namespace

DistanceTransform::DistanceTransform() : DistanceTransform(0.05f, 512, Eigen::Vector3f::Zero()) {}

DistanceTransform::DistanceTransform(float voxel_size, size_t resolution, const Eigen::Vector3f& origin)
    : GeometryBase3D(GeometryType::DistanceTransform), voxel_size_(voxel_size), resolution_((int)resolution), origin_(origin) {}

DistanceTransform::~DistanceTransform() {
    if (dt_) (void)mi_icp_dt_destroy(Engine(), dt_);
}

mi_icp_dt* DistanceTransform::Handle() const {
    if (!dt_) {
        Check(mi_icp_dt_create(Engine(), resolution_, &dt_));
        made_resolution_ = resolution_;
    } else if (made_resolution_ != resolution_) {
        const int rc = mi_icp_dt_reconstruct(Engine(), dt_, resolution_);
        if (rc == MI_ICP_ERR_HIP) dt_ = nullptr;  // (the planes could not be made: the handle is gone)
        Check(rc);
        made_resolution_ = resolution_;
    }
    return dt_;
}

DistanceTransform& DistanceTransform::Clear() {
    if (dt_ && made_resolution_ == resolution_) Check(mi_icp_dt_compute_cells(Engine(), dt_, nullptr, 0, nullptr));
    return *this;
}

Eigen::Vector3f DistanceTransform::GetMinBound() const {
    const float len = voxel_size_ * (float)resolution_ * 0.5f;
    return origin_ - Eigen::Vector3f(len, len, len);
}

Eigen::Vector3f DistanceTransform::GetMaxBound() const {
    const float len = voxel_size_ * (float)resolution_ * 0.5f;
    return origin_ + Eigen::Vector3f(len, len, len);
}

AxisAlignedBoundingBox3 DistanceTransform::GetAxisAlignedBoundingBox() const {
    return AxisAlignedBoundingBox3(GetMinBound(), GetMaxBound());
}

DistanceTransform& DistanceTransform::Transform(const Eigen::Matrix4f&) {
    LogError("DenseGrid::Transform is not supported");
    return *this;
}

DistanceTransform& DistanceTransform::Rotate(const Eigen::Matrix3f&, bool) {
    LogError("DenseGrid::Rotate is not supported");
    return *this;
}

DistanceTransform& DistanceTransform::Translate(const Eigen::Vector3f& translation, bool relative) {
    origin_ = relative ? origin_ + translation : translation;
    return *this;
}

DistanceTransform& DistanceTransform::Scale(const float scale, bool) {
    voxel_size_ *= scale;
    return *this;
}

DistanceTransform& DistanceTransform::Reconstruct(float voxel_size, size_t resolution) {
    voxel_size_ = voxel_size;
    resolution_ = (int)resolution;
    if (dt_) {
        made_resolution_ = 0;  // (also for the same resolution: no sites again)
        (void)Handle();
    }
    return *this;
}

DistanceTransform& DistanceTransform::ComputeEDT(const utility::device_vector<Eigen::Vector3i>& points) {
    Check(mi_icp_dt_compute_cells(Engine(), Handle(), points.empty() ? nullptr : points.data()->data(), (int64_t)points.size(),
                                  nullptr));
    Check(mi_icp_synchronize(Engine()));
    return *this;
}

DistanceTransform& DistanceTransform::ComputeEDT(const VoxelGrid& voxelgrid) {
    if (std::abs(voxel_size_ - voxelgrid.voxel_size_) > FLT_EPSILON) {  // distancetransform.cu:332-337
        LogError("Unsupport computing Voronoi diagrams from different voxel size.");
        return *this;
    }
    const auto& keys = voxelgrid.voxels_keys_;
    Check(mi_icp_dt_compute_voxelgrid(Engine(), Handle(), voxel_size_, origin_.data(), keys.empty() ? nullptr : keys.data()->data(),
                                      (int64_t)keys.size(), voxelgrid.voxel_size_, voxelgrid.origin_.data(), nullptr));
    Check(mi_icp_synchronize(Engine()));
    return *this;
}

DistanceTransform& DistanceTransform::ComputeVoronoiDiagram(const utility::device_vector<Eigen::Vector3i>& points) {
    return ComputeEDT(points);
}

DistanceTransform& DistanceTransform::ComputeVoronoiDiagram(const VoxelGrid& voxelgrid) { return ComputeEDT(voxelgrid); }

std::unique_ptr<utility::device_vector<float>> DistanceTransform::GetDistances(
        const utility::device_vector<Eigen::Vector3f>& queries) const {
    auto out = std::make_unique<utility::device_vector<float>>(queries.size());
    if (queries.empty()) return out;
    Check(mi_icp_dt_query(Engine(), Handle(), voxel_size_, origin_.data(), Ptr(queries), (int64_t)queries.size(), out->data(),
                          nullptr));
    Check(mi_icp_synchronize(Engine()));
    return out;
}

std::tuple<bool, DistanceVoxel> DistanceTransform::GetVoxel(const Eigen::Vector3f& point) const {
    utility::device_vector<Eigen::Vector3f> pt(std::vector<Eigen::Vector3f>{point});
    utility::device_vector<float> dist(1);
    utility::device_vector<Eigen::Vector3i> idx(1);
    Check(mi_icp_dt_query(Engine(), Handle(), voxel_size_, origin_.data(), Ptr(pt), 1, dist.data(), idx.data()->data()));
    Check(mi_icp_synchronize(Engine()));
    const float d = dist.to_host()[0];
    if (std::isnan(d)) return std::make_tuple(false, DistanceVoxel());
    return std::make_tuple(true, MakeDistanceVoxel(idx.to_host()[0], d));
}

float DistanceTransform::GetDistance(const Eigen::Vector3f& query) const {
    const auto r = GetVoxel(query);
    return std::get<0>(r) ? std::get<1>(r).distance_ : std::numeric_limits<float>::quiet_NaN();
}

std::vector<DistanceVoxel> DistanceTransform::GetVoxels() const {
    const size_t n = (size_t)resolution_ * (size_t)resolution_ * (size_t)resolution_;
    mi_icp_dt* h = Handle();
    utility::device_vector<Eigen::Vector3i> idx(n);
    utility::device_vector<float> dist(n);
    Check(mi_icp_dt_get_voxels(Engine(), h, voxel_size_, idx.data()->data(), dist.data()));
    const std::vector<Eigen::Vector3i> hi = idx.to_host();
    const std::vector<float> hd = dist.to_host();
    std::vector<DistanceVoxel> out;
    out.reserve(n);
    for (size_t i = 0; i < n; ++i) out.push_back(MakeDistanceVoxel(hi[i], hd[i]));
    return out;
}

std::shared_ptr<DistanceTransform> DistanceTransform::CreateFromOccupancyGrid(const OccupancyGrid& input) {
    if (input.voxel_size_ <= 0.0f) LogError("[CreateOccupancyGrid] occupancy grid  voxel_size <= 0.");  // distancetransform_factory.cu:42-45
    auto output = std::make_shared<DistanceTransform>(input.voxel_size_, (size_t)input.resolution_, input.origin_);
    Check(mi_icp_dt_compute_occgrid(Engine(), output->Handle(), input.Handle(), input.occ_prob_thres_log_));
    return output;
}

}  // namespace geometry

// ---------------------------------------------------------------- integration
// ---------------------------------------------------------------- collision (collision.cu, primitives.cu) over mi_icp_collision_*
namespace collision {

namespace {

using geometry::KeyPtr;

mi_icp_primitive Record(const PrimitivePack& p) {
    mi_icp_primitive r;
    static_assert(sizeof(r) == sizeof(p), "one layout");
    std::memcpy(&r, &p, sizeof(r));
    return r;
}

// a side of a call and whatever device memory it needs for the call's duration
struct Side {
    mi_icp_collision_side s;
    utility::device_vector<PrimitivePack> records;
    Side() { std::memset(&s, 0, sizeof(s)); }
};

void Fill(Side* d, const geometry::VoxelGrid& g) {
    d->s.kind = MI_ICP_COLLISION_VOXELGRID;
    d->s.keys = KeyPtr(g.voxels_keys_);
    d->s.m = (int64_t)g.voxels_keys_.size();
    d->s.keys_sorted = g.KeysSorted() ? 1 : 0;
    d->s.voxel_size = g.voxel_size_;
    for (int k = 0; k < 3; ++k) d->s.origin[k] = g.origin_(k);
}
void Fill(Side* d, const geometry::OccupancyGrid& g) {
    d->s.kind = MI_ICP_COLLISION_OCCGRID;
    d->s.grid = g.Handle();
    d->s.grid_params = geometry::OccParams(g);
}
void Fill(Side* d, const geometry::LineSet<3>& l) {
    d->s.kind = MI_ICP_COLLISION_LINESET;
    d->s.points = l.points_.empty() ? nullptr : l.points_.data()->data();
    d->s.n_points = (int64_t)l.points_.size();
    d->s.lines = l.lines_.empty() ? nullptr : l.lines_.data()->data();
    d->s.n_lines = (int64_t)l.lines_.size();
}
void Fill(Side* d, const PrimitiveArray& p) {
    d->records = p;
    d->s.kind = MI_ICP_COLLISION_PRIMITIVES;
    d->s.primitives = p.empty() ? nullptr : reinterpret_cast<const mi_icp_primitive*>(d->records.data());
    d->s.n_primitives = (int64_t)p.size();
}

CollisionResult::CollisionType TypeOf(const geometry::VoxelGrid&) { return CollisionResult::CollisionType::VoxelGrid; }
CollisionResult::CollisionType TypeOf(const geometry::OccupancyGrid&) { return CollisionResult::CollisionType::OccupancyGrid; }
CollisionResult::CollisionType TypeOf(const geometry::LineSet<3>&) { return CollisionResult::CollisionType::LineSet; }
CollisionResult::CollisionType TypeOf(const PrimitiveArray&) { return CollisionResult::CollisionType::Primitives; }

// the capacity rule: once for the count, again with room; a refusal logs and gives no pairs
std::shared_ptr<CollisionResult> Run(const Side& a, const Side& b, float margin, CollisionResult::CollisionType ta,
                                     CollisionResult::CollisionType tb) {
    auto out = std::make_shared<CollisionResult>(ta, tb);
    int64_t m = 0;
    if (geometry::Refused(mi_icp_collision_compute(Engine(), &a.s, &b.s, margin, nullptr, 0, &m)) || m == 0) return out;
    out->collision_index_pairs_.resize((size_t)m);
    Check(mi_icp_collision_compute(Engine(), &a.s, &b.s, margin, out->collision_index_pairs_.data()->data(), m, &m));
    Check(mi_icp_synchronize(Engine()));
    out->collision_index_pairs_.resize((size_t)m);
    return out;
}

template <class A, class B>
std::shared_ptr<CollisionResult> Intersect(const A& a, const B& b, float margin) {
    Side sa, sb;
    Fill(&sa, a);
    Fill(&sb, b);
    return Run(sa, sb, margin, TypeOf(a), TypeOf(b));
}

utility::device_vector<size_t> Column(const utility::device_vector<Eigen::Vector2i>& pairs, int col) {
    const std::vector<Eigen::Vector2i> h = pairs.to_host();
    std::vector<size_t> out(h.size());
    for (size_t i = 0; i < h.size(); ++i) out[i] = (size_t)h[i](col);
    return utility::device_vector<size_t>(out);
}

}  // namespace

utility::device_vector<size_t> CollisionResult::GetFirstCollisionIndices() const { return Column(collision_index_pairs_, 0); }
utility::device_vector<size_t> CollisionResult::GetSecondCollisionIndices() const { return Column(collision_index_pairs_, 1); }

#define CUPOCH_AMD_INTERSECTION(A, B) \
    std::shared_ptr<CollisionResult> ComputeIntersection(const A& a, const B& b, float margin) { return Intersect(a, b, margin); }
CUPOCH_AMD_INTERSECTION(geometry::VoxelGrid, geometry::VoxelGrid)
CUPOCH_AMD_INTERSECTION(geometry::VoxelGrid, geometry::LineSet<3>)
CUPOCH_AMD_INTERSECTION(geometry::LineSet<3>, geometry::VoxelGrid)
CUPOCH_AMD_INTERSECTION(geometry::VoxelGrid, geometry::OccupancyGrid)
CUPOCH_AMD_INTERSECTION(geometry::OccupancyGrid, geometry::VoxelGrid)
CUPOCH_AMD_INTERSECTION(geometry::LineSet<3>, geometry::OccupancyGrid)
CUPOCH_AMD_INTERSECTION(geometry::OccupancyGrid, geometry::LineSet<3>)
CUPOCH_AMD_INTERSECTION(PrimitiveArray, geometry::VoxelGrid)
CUPOCH_AMD_INTERSECTION(geometry::VoxelGrid, PrimitiveArray)
CUPOCH_AMD_INTERSECTION(PrimitiveArray, geometry::OccupancyGrid)
CUPOCH_AMD_INTERSECTION(geometry::OccupancyGrid, PrimitiveArray)
#undef CUPOCH_AMD_INTERSECTION

// Intersection<TargetT>: an unsorted VoxelGrid target is sorted once, here
template <>
void Intersection<geometry::VoxelGrid>::Construct() {
    const size_t m = target_.voxels_keys_.size();
    if (target_.KeysSorted() || m < 2) return;
    sorted_keys_.resize(m);
    sorted_index_.resize(m);
    int64_t mo = 0;
    Check(mi_icp_collision_sort_keys(Engine(), KeyPtr(target_.voxels_keys_), (int64_t)m, KeyPtr(sorted_keys_), sorted_index_.data(), &mo));
    sorted_keys_.resize((size_t)mo);
    sorted_index_.resize((size_t)mo);
}
template <>
void Intersection<geometry::OccupancyGrid>::Construct() {}

namespace {
template <class T>
void FillTarget(Side* d, const Intersection<T>& it) {
    Fill(d, it.target_);
}
template <>
void FillTarget(Side* d, const Intersection<geometry::VoxelGrid>& it) {
    Fill(d, it.target_);
    if (it.sorted_keys_.empty()) return;
    d->s.keys = KeyPtr(it.sorted_keys_);
    d->s.keys_index = it.sorted_index_.data();
    d->s.m = (int64_t)it.sorted_keys_.size();
    d->s.keys_sorted = 1;
}
}  // namespace

template <typename TargetT>
template <typename QueryT>
std::shared_ptr<CollisionResult> Intersection<TargetT>::Compute(const QueryT& query, float margin) const {
    Side sa, sb;
    FillTarget(&sa, *this);
    Fill(&sb, query);
    return Run(sa, sb, margin, TypeOf(target_), TypeOf(query));
}
template std::shared_ptr<CollisionResult> Intersection<geometry::VoxelGrid>::Compute(const geometry::VoxelGrid&, float) const;
template std::shared_ptr<CollisionResult> Intersection<geometry::VoxelGrid>::Compute(const geometry::LineSet<3>&, float) const;
template std::shared_ptr<CollisionResult> Intersection<geometry::VoxelGrid>::Compute(const geometry::OccupancyGrid&, float) const;
template std::shared_ptr<CollisionResult> Intersection<geometry::VoxelGrid>::Compute(const PrimitiveArray&, float) const;
template std::shared_ptr<CollisionResult> Intersection<geometry::OccupancyGrid>::Compute(const geometry::VoxelGrid&, float) const;
template std::shared_ptr<CollisionResult> Intersection<geometry::OccupancyGrid>::Compute(const geometry::LineSet<3>&, float) const;
template std::shared_ptr<CollisionResult> Intersection<geometry::OccupancyGrid>::Compute(const PrimitiveArray&, float) const;

geometry::AxisAlignedBoundingBox3 Primitive::GetAxisAlignedBoundingBox() const {
    const mi_icp_primitive r = Record(PrimitivePack(*this));
    Eigen::Vector3f mn, mx;
    Check(mi_icp_primitive_aabb(&r, mn.data(), mx.data()));
    return geometry::AxisAlignedBoundingBox3(mn, mx);
}

std::shared_ptr<geometry::VoxelGrid> CreateVoxelGrid(const Primitive& primitive, float voxel_size) {
    auto output = std::make_shared<geometry::VoxelGrid>();
    const mi_icp_primitive r = Record(PrimitivePack(primitive));
    int64_t m = 0;
    Eigen::Vector3f origin;
    if (geometry::Refused(mi_icp_collision_voxelize_primitive(Engine(), &r, voxel_size, nullptr, nullptr, 0, &m, origin.data()))) return output;
    output->voxel_size_ = voxel_size;
    output->origin_ = origin;
    if (m == 0) return output;
    utility::device_vector<Eigen::Vector3i> ok((size_t)m);
    utility::device_vector<Eigen::Vector3f> oc((size_t)m);
    Check(mi_icp_collision_voxelize_primitive(Engine(), &r, voxel_size, KeyPtr(ok), geometry::ColPtr(oc), m, &m, origin.data()));
    geometry::SetVoxelArrays(output.get(), ok, oc, (size_t)m);
    return output;
}

}  // namespace collision

// ---------------------------------------------------------------- geometry::Graph<3> (graph.cu, graph_factory.cu) over mi_icp_graph_*
namespace geometry {

namespace {
int* LinePtr(utility::device_vector<Eigen::Vector2i>& v) { return v.empty() ? nullptr : v.data()->data(); }
const int* LinePtr(const utility::device_vector<Eigen::Vector2i>& v) { return v.empty() ? nullptr : v.data()->data(); }
float* Vec3Ptr(utility::device_vector<Eigen::Vector3f>& v) { return v.empty() ? nullptr : v.data()->data(); }

template <class T>
void Append(utility::device_vector<T>* dst, const utility::device_vector<T>& src) {
    const size_t n = dst->size();
    dst->resize(n + src.size());
    if (src.size()) utility::copy_d2d(dst->data() + n, src.data(), src.size() * sizeof(T));
}

// every line has a weight: missing ones are 1.0
void FillWeights(Graph<3>* g) {
    const size_t m = g->lines_.size(), have = g->edge_weights_.size();
    if (have == m) return;
    std::vector<float> w = g->edge_weights_.to_host();
    w.resize(m, 1.0f);
    g->edge_weights_ = w;
}
}  // namespace

LineSet<3>::LineSet(GeometryType type) : GeometryBase3D(type) {}

Graph<3>::Graph() : LineSet<3>(GeometryType::Graph) {}
Graph<3>::Graph(const utility::device_vector<Eigen::Vector3f>& points) : LineSet<3>(GeometryType::Graph) { points_ = points; }
Graph<3>::Graph(const thrust::host_vector<Eigen::Vector3f>& points) : LineSet<3>(GeometryType::Graph) { points_ = points; }
Graph<3>::Graph(const Graph& other)
    : LineSet<3>(GeometryType::Graph),
      edge_index_offsets_(other.edge_index_offsets_),
      edge_weights_(other.edge_weights_),
      node_colors_(other.node_colors_),
      is_directed_(other.is_directed_),
      sorted_(other.sorted_) {
    points_ = other.points_;
    lines_ = other.lines_;
    colors_ = other.colors_;
}
Graph<3>::~Graph() {}

Graph<3>& Graph<3>::Clear() {
    LineSet<3>::Clear();
    edge_index_offsets_.clear();
    edge_weights_.clear();
    node_colors_.clear();
    sorted_ = false;
    return *this;
}

Graph<3>& Graph<3>::ConstructGraph(bool set_edge_weights_from_distance) {
    if (lines_.empty()) {
        LogError("[ConstructGraph] Graph has no edges.");
        return *this;
    }
    FillWeights(this);
    edge_index_offsets_.resize(points_.size() + 1);
    Check(mi_icp_graph_construct(Engine(), LinePtr(lines_), edge_weights_.data(), HasColors() ? Vec3Ptr(colors_) : nullptr,
                                 (int64_t)lines_.size(), (int64_t)points_.size(), edge_index_offsets_.data()));
    sorted_ = true;
    if (set_edge_weights_from_distance) SetEdgeWeightsFromDistance();
    return *this;
}

Graph<3>& Graph<3>::SetEdgeWeightsFromDistance() {
    edge_weights_.resize(lines_.size());
    Check(mi_icp_graph_weights_from_distance(Engine(), Vec3Ptr(points_), (int64_t)points_.size(), LinePtr(lines_), (int64_t)lines_.size(),
                                             edge_weights_.data()));
    return *this;
}

Graph<3>& Graph<3>::SetEdgeWeights(const utility::device_vector<Eigen::Vector2i>& edges, float weight) {
    if (lines_.empty() || edges.empty()) return *this;
    if (!IsConstructed()) ConstructGraph(false);
    Check(mi_icp_graph_set_edge_weights(Engine(), LinePtr(lines_), edge_weights_.data(), (int64_t)lines_.size(), LinePtr(edges),
                                        (int64_t)edges.size(), is_directed_ ? 1 : 0, weight));
    Check(mi_icp_synchronize(Engine()));
    return *this;
}

Graph<3>& Graph<3>::AddEdges(const utility::device_vector<Eigen::Vector2i>& edges, const utility::device_vector<float>& weights, bool lazy_add) {
    if (!weights.empty() && edges.size() != weights.size()) {
        LogError("[AddEdges] edges size is not equal to weights size.");
        return *this;
    }
    FillWeights(this);
    const bool had_colors = HasColors();
    std::vector<Eigen::Vector2i> e = edges.to_host();
    std::vector<float> w = weights.empty() ? std::vector<float>(e.size(), 1.0f) : weights.to_host();  // (the reference's resize here is wrong)
    if (!is_directed_) {
        const size_t k = e.size();
        for (size_t i = 0; i < k; ++i) {
            e.push_back(Eigen::Vector2i(e[i](1), e[i](0)));
            w.push_back(w[i]);
        }
    }
    Append(&lines_, utility::device_vector<Eigen::Vector2i>(e));
    Append(&edge_weights_, utility::device_vector<float>(w));
    if (had_colors) Append(&colors_, utility::device_vector<Eigen::Vector3f>(std::vector<Eigen::Vector3f>(e.size(), Eigen::Vector3f(1.0f, 1.0f, 1.0f))));
    sorted_ = false;
    return lazy_add ? *this : ConstructGraph(false);
}
Graph<3>& Graph<3>::AddEdges(const thrust::host_vector<Eigen::Vector2i>& edges, const thrust::host_vector<float>& weights, bool lazy_add) {
    return AddEdges(utility::device_vector<Eigen::Vector2i>(edges), utility::device_vector<float>(weights), lazy_add);
}
Graph<3>& Graph<3>::AddEdge(const Eigen::Vector2i& edge, float weight, bool lazy_add) {
    return AddEdges(std::vector<Eigen::Vector2i>{edge}, std::vector<float>{weight}, lazy_add);
}

Graph<3>& Graph<3>::RemoveEdges(const utility::device_vector<Eigen::Vector2i>& edges) {
    if (lines_.empty()) return *this;
    if (!IsConstructed()) ConstructGraph(false);
    const bool has_colors = HasColors();
    int64_t m = 0;
    edge_index_offsets_.resize(points_.size() + 1);
    Check(mi_icp_graph_remove_edges(Engine(), LinePtr(lines_), edge_weights_.data(), has_colors ? Vec3Ptr(colors_) : nullptr,
                                    (int64_t)lines_.size(), (int64_t)points_.size(), LinePtr(edges), (int64_t)edges.size(),
                                    is_directed_ ? 1 : 0, edge_index_offsets_.data(), &m));
    Check(mi_icp_synchronize(Engine()));
    lines_.resize((size_t)m);
    edge_weights_.resize((size_t)m);
    if (has_colors) colors_.resize((size_t)m);
    return *this;
}
Graph<3>& Graph<3>::RemoveEdges(const thrust::host_vector<Eigen::Vector2i>& edges) { return RemoveEdges(utility::device_vector<Eigen::Vector2i>(edges)); }
Graph<3>& Graph<3>::RemoveEdge(const Eigen::Vector2i& edge) { return RemoveEdges(std::vector<Eigen::Vector2i>{edge}); }

Graph<3>& Graph<3>::AddNodeAndConnect(const Eigen::Vector3f& point, float max_edge_distance, bool lazy_add) {
    const size_t n = points_.size();
    std::vector<Eigen::Vector2i> e;
    std::vector<float> w;
    if (n) {
        utility::device_vector<float> d(n);
        Check(mi_icp_graph_node_distances(Engine(), Vec3Ptr(points_), (int64_t)n, point.data(), d.data()));
        Check(mi_icp_synchronize(Engine()));
        const std::vector<float> h = d.to_host();
        for (size_t i = 0; i < n; ++i)
            if (h[i] < max_edge_distance) {  // strictly nearer
                e.push_back(Eigen::Vector2i((int)i, (int)n));
                w.push_back(h[i]);
            }
    }
    Append(&points_, utility::device_vector<Eigen::Vector3f>(std::vector<Eigen::Vector3f>{point}));
    if (!node_colors_.empty()) Append(&node_colors_, utility::device_vector<Eigen::Vector3f>(std::vector<Eigen::Vector3f>{Eigen::Vector3f(1.0f, 1.0f, 1.0f)}));
    sorted_ = false;
    if (e.empty()) return (lazy_add || lines_.empty()) ? *this : ConstructGraph(false);
    return AddEdges(e, w, lazy_add);
}

Graph<3>& Graph<3>::ConnectToNearestNeighbors(float max_edge_distance, size_t max_num_edges) {
    const size_t n = points_.size();
    if (n == 0) return *this;
    const int knn = (int)max_num_edges + 1;
    if (knn < 1 || knn > 100) {
        LogError("[ConnectToNearestNeighbors] max_num_edges + 1 must be in [1, 100].");
        return *this;
    }
    knn::KDTreeFlann tree(points_);
    utility::device_vector<int> di;
    utility::device_vector<float> dd;
    if (tree.SearchRadius(points_, max_edge_distance, knn, di, dd) < 0) return *this;
    const std::vector<int> idx = di.to_host();
    std::vector<uint64_t> keys;  // first * n + second: the row is the query
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < knn; ++k) {
            const int j = idx[i * (size_t)knn + (size_t)k];
            if (j < 0 || (size_t)j == i) continue;
            keys.push_back((uint64_t)i * n + (uint64_t)j);
            if (!is_directed_) keys.push_back((uint64_t)j * n + (uint64_t)i);
        }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::vector<uint64_t> have;
    for (const auto& l : lines_.to_host()) have.push_back((uint64_t)l(0) * n + (uint64_t)l(1));
    std::sort(have.begin(), have.end());
    std::vector<Eigen::Vector2i> fresh;
    for (uint64_t k : keys)
        if (!std::binary_search(have.begin(), have.end(), k)) fresh.push_back(Eigen::Vector2i((int)(k / n), (int)(k % n)));
    FillWeights(this);
    const bool had_colors = HasColors();
    utility::device_vector<Eigen::Vector2i> dl(fresh);
    utility::device_vector<float> dw(fresh.size());
    Check(mi_icp_graph_weights_from_distance(Engine(), Vec3Ptr(points_), (int64_t)n, LinePtr(dl), (int64_t)dl.size(), dw.data()));
    Append(&lines_, dl);
    Append(&edge_weights_, dw);
    if (had_colors) Append(&colors_, utility::device_vector<Eigen::Vector3f>(std::vector<Eigen::Vector3f>(fresh.size(), Eigen::Vector3f(1.0f, 1.0f, 1.0f))));
    sorted_ = false;
    return ConstructGraph(false);
}

Graph<3>& Graph<3>::PaintEdgesColor(const thrust::host_vector<Eigen::Vector2i>& edges, const Eigen::Vector3f& color) {
    std::vector<Eigen::Vector3f> c = HasColors() ? colors_.to_host() : std::vector<Eigen::Vector3f>(lines_.size(), Eigen::Vector3f(1.0f, 1.0f, 1.0f));
    const std::vector<Eigen::Vector2i> l = lines_.to_host();
    for (size_t i = 0; i < l.size(); ++i)
        for (const auto& e : edges)
            if ((l[i](0) == e(0) && l[i](1) == e(1)) || (!is_directed_ && l[i](0) == e(1) && l[i](1) == e(0))) c[i] = color;
    colors_ = c;
    return *this;
}
Graph<3>& Graph<3>::PaintEdgeColor(const Eigen::Vector2i& edge, const Eigen::Vector3f& color) {
    return PaintEdgesColor(std::vector<Eigen::Vector2i>{edge}, color);
}
Graph<3>& Graph<3>::PaintNodesColor(const thrust::host_vector<int>& nodes, const Eigen::Vector3f& color) {
    std::vector<Eigen::Vector3f> c = HasNodeColors() ? node_colors_.to_host() : std::vector<Eigen::Vector3f>(points_.size(), Eigen::Vector3f(1.0f, 1.0f, 1.0f));
    for (int i : nodes)
        if (i >= 0 && (size_t)i < c.size()) c[(size_t)i] = color;
    node_colors_ = c;
    return *this;
}
Graph<3>& Graph<3>::PaintNodeColor(int node, const Eigen::Vector3f& color) { return PaintNodesColor(std::vector<int>{node}, color); }

std::shared_ptr<Graph<3>::SSSPResultHostArray> Graph<3>::DijkstraPathsHost(int start_node_index, int end_node_index) const {
    auto out = std::make_shared<SSSPResultHostArray>(points_.size());
    if (!IsConstructed()) {
        LogError("[DijkstraPath] this graph is not constructed.");
        return out;
    }
    const size_t n = points_.size();
    utility::device_vector<float> d(n);
    utility::device_vector<int> p(n);
    Check(mi_icp_graph_sssp(Engine(), edge_index_offsets_.data(), LinePtr(lines_), edge_weights_.data(), (int64_t)n, (int64_t)lines_.size(),
                            start_node_index, end_node_index, d.data(), p.data(), nullptr));
    Check(mi_icp_synchronize(Engine()));
    const std::vector<float> hd = d.to_host();
    const std::vector<int> hp = p.to_host();
    for (size_t i = 0; i < n; ++i) (*out)[i] = SSSPResult(hd[i], hp[i]);
    return out;
}
std::shared_ptr<Graph<3>::SSSPResultArray> Graph<3>::DijkstraPaths(int start_node_index, int end_node_index) const {
    auto out = std::make_shared<SSSPResultArray>();
    *out = *DijkstraPathsHost(start_node_index, end_node_index);
    return out;
}
std::pair<std::shared_ptr<thrust::host_vector<int>>, float> Graph<3>::DijkstraPath(int start_node_index, int end_node_index) const {
    auto nodes = std::make_shared<thrust::host_vector<int>>();
    const float inf = std::numeric_limits<float>::infinity();
    if (end_node_index < 0 || (size_t)end_node_index >= points_.size()) return std::make_pair(nodes, inf);
    const auto res = DijkstraPathsHost(start_node_index, end_node_index);
    if ((*res)[(size_t)end_node_index].prev_index_ < 0) return std::make_pair(nodes, inf);
    int v = end_node_index;
    nodes->push_back(v);
    while (v != start_node_index && nodes->size() <= res->size()) {
        v = (*res)[(size_t)v].prev_index_;
        nodes->push_back(v);
    }
    std::reverse(nodes->begin(), nodes->end());
    return std::make_pair(nodes, (*res)[(size_t)end_node_index].shortest_distance_);
}

std::shared_ptr<Graph<3>> Graph<3>::CreateFromAxisAlignedBoundingBox(const AxisAlignedBoundingBox3& bbox, const Eigen::Vector3i& resolutions) {
    return CreateFromAxisAlignedBoundingBox(bbox.GetMinBound(), bbox.GetMaxBound(), resolutions);
}
std::shared_ptr<Graph<3>> Graph<3>::CreateFromAxisAlignedBoundingBox(const Eigen::Vector3f& min_bound, const Eigen::Vector3f& max_bound,
                                                                     const Eigen::Vector3i& resolutions) {
    auto out = std::make_shared<Graph<3>>();
    int64_t n = 0, m = 0;
    const int32_t res[3] = {resolutions(0), resolutions(1), resolutions(2)};
    if (Refused(mi_icp_graph_lattice(Engine(), min_bound.data(), max_bound.data(), res, nullptr, 0, nullptr, nullptr, 0, nullptr, &n, &m))) return out;
    out->points_.resize((size_t)n);
    out->lines_.resize((size_t)m);
    out->edge_weights_.resize((size_t)m);
    out->edge_index_offsets_.resize((size_t)n + 1);
    Check(mi_icp_graph_lattice(Engine(), min_bound.data(), max_bound.data(), res, Vec3Ptr(out->points_), n, LinePtr(out->lines_),
                               out->edge_weights_.data(), m, out->edge_index_offsets_.data(), &n, &m));
    Check(mi_icp_synchronize(Engine()));
    out->sorted_ = true;
    return out;
}

}  // namespace geometry

// ---------------------------------------------------------------- planning (planner.cu)
namespace planning {

Pos3DPlanner::Pos3DPlanner(const geometry::Graph<3>& graph, float object_radius, float max_edge_distance)
    : graph_(graph), object_radius_(object_radius), max_edge_distance_(max_edge_distance) {}
Pos3DPlanner::~Pos3DPlanner() {}
Pos3DPlanner::Pos3DPlanner(const Pos3DPlanner& other)
    : PlannerBase(other), graph_(other.graph_), object_radius_(other.object_radius_), max_edge_distance_(other.max_edge_distance_) {}

Pos3DPlanner& Pos3DPlanner::UpdateGraph() {
    RemoveCollisionEdges(graph_);
    return *this;
}

void Pos3DPlanner::RemoveCollisionEdges(geometry::Graph<3>& graph) const {
    graph.SetEdgeWeightsFromDistance();
    for (const auto& obstacle : obstacles_) {
        std::shared_ptr<collision::CollisionResult> res;
        const geometry::LineSet<3>& lines = graph;
        switch (obstacle->GetGeometryType()) {
            case geometry::Geometry::GeometryType::VoxelGrid:
                res = collision::ComputeIntersection((const geometry::VoxelGrid&)(*obstacle), lines, object_radius_);
                break;
            case geometry::Geometry::GeometryType::OccupancyGrid:
                res = collision::ComputeIntersection((const geometry::OccupancyGrid&)(*obstacle), lines, object_radius_);
                break;
            default: LogError("Unsupported obstacle type.");
        }
        if (!res || !res->IsCollided()) continue;
        const std::vector<Eigen::Vector2i> pairs = res->collision_index_pairs_.to_host(), all = graph.lines_.to_host();
        std::vector<Eigen::Vector2i> hit;
        for (const auto& p : pairs) hit.push_back(all[(size_t)p(1)]);
        graph.SetEdgeWeights(utility::device_vector<Eigen::Vector2i>(hit), std::numeric_limits<float>::infinity());
    }
}

std::shared_ptr<Path> Pos3DPlanner::FindPath(const Eigen::Vector3f& start, const Eigen::Vector3f& goal) const {
    auto out = std::make_shared<Path>();
    geometry::Graph<3> g = graph_;
    const size_t n = g.points_.size();
    g.AddNodeAndConnect(start, max_edge_distance_, true);
    g.AddNodeAndConnect(goal, max_edge_distance_, false);
    if (!g.IsConstructed()) return out;  // (no edge reached either node)
    RemoveCollisionEdges(g);
    const auto path = g.DijkstraPath((int)n, (int)n + 1);
    if (std::isinf(path.second)) return out;
    const std::vector<Eigen::Vector3f> pts = g.points_.to_host();
    for (int i : *path.first) out->push_back(pts[(size_t)i]);
    return out;
}

}  // namespace planning

namespace integration {

UniformTSDFVolume::UniformTSDFVolume(float length, int resolution, float sdf_trunc, TSDFVolumeColorType color_type,
                                     const Eigen::Vector3f& origin)
    : TSDFVolume(length / (float)resolution, sdf_trunc, color_type),
      origin_(origin),
      length_(length),
      resolution_(resolution),
      voxel_num_(resolution * resolution * resolution) {
    Check(mi_icp_tsdf_create(Engine(), length, resolution, sdf_trunc, (int)color_type, origin_.data(), &volume_));
}

UniformTSDFVolume::~UniformTSDFVolume() {
    if (volume_) (void)mi_icp_tsdf_destroy(Engine(), volume_);
}

void UniformTSDFVolume::Reset() { Check(mi_icp_tsdf_reset(Engine(), volume_)); }

namespace {
// mi_icp_tsdf_integrate or mi_icp_stsdf_integrate (`tail`: what the one takes after the extrinsic) on an RGBDImage and
// an intrinsic, described as the C ABI takes them; no colour image goes to a volume without colour
template <class Vol, class... Tail>
int IntegrateFrame(int (*integrate)(mi_icp_ctx*, Vol*, const void*, int, int, int, int, const void*, int, int, int, int, int, int,
                                    const float*, const float*, Tail...),
                   Vol* volume, const geometry::RGBDImage& image, const camera::PinholeCameraIntrinsic& intrinsic,
                   const Eigen::Matrix4f& extrinsic, TSDFVolumeColorType color_type, Tail... tail) {
    const geometry::Image &d = image.depth_, &c = image.color_;
    const float k4[4] = {intrinsic.fx_, intrinsic.fy_, intrinsic.cx_, intrinsic.cy_};
    const bool colored = color_type != TSDFVolumeColorType::NoColor;
    return integrate(Engine(), volume, d.data_.empty() ? nullptr : d.data_.data(), d.width_, d.height_, d.num_of_channels_,
                     d.bytes_per_channel_, (!colored || c.data_.empty()) ? nullptr : c.data_.data(), c.width_, c.height_,
                     c.num_of_channels_, c.bytes_per_channel_, intrinsic.width_, intrinsic.height_, k4, extrinsic.data(), tail...);
}
}  // namespace

void UniformTSDFVolume::Integrate(const geometry::RGBDImage& image, const camera::PinholeCameraIntrinsic& intrinsic,
                                  const Eigen::Matrix4f& extrinsic) {
    (void)TryIntegrate(image, intrinsic, extrinsic);
}

bool UniformTSDFVolume::TryIntegrate(const geometry::RGBDImage& image, const camera::PinholeCameraIntrinsic& intrinsic,
                                     const Eigen::Matrix4f& extrinsic) {
    const int rc = IntegrateFrame(mi_icp_tsdf_integrate, volume_, image, intrinsic, extrinsic, color_type_, (int)MI_ICP_DEVICE);
    if (rc == MI_ICP_ERR_INVALID) {  // uniform_tsdfvolume.cu:677-695
        LogError("[UniformTSDFVolume::Integrate] Unsupported image format.");
        return false;
    }
    Check(rc);
    return true;
}

namespace {
// the capacity rule of include/mi_icp.h: fill when it fits, else make room for the count that came back and call again
constexpr size_t kFirstCapacity = (size_t)1 << 18;  // points an extraction makes room for before it knows the count

template <class Call>
std::shared_ptr<geometry::PointCloud> FillCloud(bool normals, bool colors, size_t capacity, Call call) {
    auto out = std::make_shared<geometry::PointCloud>();
    int64_t m = 0;
    for (int pass = 0; pass < 2; ++pass) {
        out->points_.resize(capacity);
        if (normals) out->normals_.resize(capacity);
        if (colors) out->colors_.resize(capacity);
        Check(call(capacity ? out->points_.data()->data() : nullptr,
                   (capacity && normals) ? out->normals_.data()->data() : nullptr,
                   (capacity && colors) ? out->colors_.data()->data() : nullptr, (int64_t)capacity, &m));
        if ((size_t)m <= capacity) break;
        capacity = (size_t)m;
    }
    out->points_.resize((size_t)m);
    if (normals) out->normals_.resize((size_t)m);
    if (colors) out->colors_.resize((size_t)m);
    return out;
}
}  // namespace

std::shared_ptr<geometry::PointCloud> UniformTSDFVolume::ExtractPointCloud() {
    mi_icp_tsdf* v = volume_;
    return FillCloud(true, color_type_ != TSDFVolumeColorType::NoColor, kFirstCapacity, [v](float* p, float* n, float* c, int64_t cap, int64_t* m) {
        return mi_icp_tsdf_extract_point_cloud(Engine(), v, p, n, c, cap, m, MI_ICP_DEVICE);
    });
}

std::shared_ptr<geometry::PointCloud> UniformTSDFVolume::ExtractVoxelPointCloud() const {
    mi_icp_tsdf* v = volume_;
    return FillCloud(false, true, kFirstCapacity, [v](float* p, float*, float* c, int64_t cap, int64_t* m) {
        return mi_icp_tsdf_extract_voxel_point_cloud(Engine(), v, p, c, cap, m, MI_ICP_DEVICE);
    });
}

std::shared_ptr<geometry::PointCloud> UniformTSDFVolume::Raycast(const camera::PinholeCameraIntrinsic& intrinsic,
                                                                 const Eigen::Matrix4f& extrinsic, float sdf_trunc,
                                                                 bool project_valid_depth_only) const {
    mi_icp_tsdf* v = volume_;
    const float k4[4] = {intrinsic.fx_, intrinsic.fy_, intrinsic.cx_, intrinsic.cy_};
    const int w = intrinsic.width_, h = intrinsic.height_;
    const size_t npix = (w > 0 && h > 0) ? (size_t)w * (size_t)h : 0;
    return FillCloud(true, true, npix, [&](float* p, float* n, float* c, int64_t cap, int64_t* m) {
        return mi_icp_tsdf_raycast(Engine(), v, w, h, k4, extrinsic.data(), sdf_trunc, project_valid_depth_only ? 1 : 0, p, n,
                                   c, cap, m, MI_ICP_DEVICE);
    });
}

std::vector<std::shared_ptr<geometry::PointCloud>> UniformTSDFVolume::RaycastLevels(const camera::PinholeCameraIntrinsic& intrinsic,
                                                                                    const Eigen::Matrix4f& extrinsic,
                                                                                    float sdf_trunc, int levels,
                                                                                    bool project_valid_depth_only) const {
    const float k4[4] = {intrinsic.fx_, intrinsic.fy_, intrinsic.cx_, intrinsic.cy_};
    const int w = intrinsic.width_, h = intrinsic.height_;
    size_t capacity = 0;  // every pixel of every level: always enough
    for (int i = 0; i < levels && i < MI_ICP_TSDF_MAX_LEVELS; ++i)
        if (w > 0 && h > 0) capacity += (size_t)(w >> i) * (size_t)(h >> i);
    utility::device_vector<Eigen::Vector3f> all[3];
    for (auto& a : all) a.resize(capacity);
    int64_t m[MI_ICP_TSDF_MAX_LEVELS] = {};
    Check(mi_icp_tsdf_raycast_levels(Engine(), volume_, levels, w, h, k4, extrinsic.data(), sdf_trunc,
                                     project_valid_depth_only ? 1 : 0, capacity ? all[0].data()->data() : nullptr,
                                     capacity ? all[1].data()->data() : nullptr, capacity ? all[2].data()->data() : nullptr,
                                     (int64_t)capacity, m));
    std::vector<std::shared_ptr<geometry::PointCloud>> out((size_t)levels);
    size_t first = 0;
    for (int i = 0; i < levels; ++i) {
        auto cloud = std::make_shared<geometry::PointCloud>();
        const size_t n = (size_t)m[i];
        utility::device_vector<Eigen::Vector3f>* dst[3] = {&cloud->points_, &cloud->normals_, &cloud->colors_};
        for (int k = 0; k < 3; ++k) {
            dst[k]->resize(n);
            if (n) utility::copy_d2d(dst[k]->data(), all[k].data() + first, n * sizeof(Eigen::Vector3f));
        }
        first += n;
        out[(size_t)i] = cloud;
    }
    return out;
}

std::vector<geometry::TSDFVoxel> UniformTSDFVolume::GetVoxels() const {
    const size_t n = (size_t)voxel_num_;
    const bool colored = color_type_ != TSDFVolumeColorType::NoColor;
    std::vector<float> t(n), w(n), c(colored ? 3 * n : 0);
    Check(mi_icp_tsdf_get_voxels(Engine(), volume_, t.data(), w.data(), colored ? c.data() : nullptr, MI_ICP_HOST));
    std::vector<geometry::TSDFVoxel> out(n);
    for (size_t i = 0; i < n; ++i) {
        out[i].tsdf_ = t[i];
        out[i].weight_ = w[i];
        if (colored) out[i].color_ = Eigen::Vector3f(c[i], c[n + i], c[2 * n + i]);
    }
    return out;
}

ScalableTSDFVolume::ScalableTSDFVolume(float voxel_length, float sdf_trunc, TSDFVolumeColorType color_type,
                                       int depth_sampling_stride, int map_size)
    : TSDFVolume(voxel_length, sdf_trunc, color_type),
      volume_unit_length_(voxel_length * 16.0f),
      resolution_(16),
      volume_unit_voxel_num_(4096),
      depth_sampling_stride_(depth_sampling_stride) {
    Check(mi_icp_stsdf_create(Engine(), voxel_length, sdf_trunc, (int)color_type, depth_sampling_stride, map_size, &volume_));
}

ScalableTSDFVolume::~ScalableTSDFVolume() {
    if (volume_) (void)mi_icp_stsdf_destroy(Engine(), volume_);
}

void ScalableTSDFVolume::Reset() { Check(mi_icp_stsdf_reset(Engine(), volume_)); }

void ScalableTSDFVolume::Integrate(const geometry::RGBDImage& image, const camera::PinholeCameraIntrinsic& intrinsic,
                                   const Eigen::Matrix4f& extrinsic) {
    const int rc = IntegrateFrame(mi_icp_stsdf_integrate, volume_, image, intrinsic, extrinsic, color_type_);
    if (rc == MI_ICP_ERR_INVALID && std::strstr(mi_icp_last_error(Engine()), "Unsupported image format")) {
        LogError("[ScalableTSDFVolume::Integrate] Unsupported image format.");  // scalable_tsdfvolume.cu:318-336
        return;
    }
    Check(rc);
}

std::shared_ptr<geometry::PointCloud> ScalableTSDFVolume::ExtractPointCloud() {
    mi_icp_stsdf* v = volume_;
    return FillCloud(true, color_type_ != TSDFVolumeColorType::NoColor, kFirstCapacity, [v](float* p, float* n, float* c, int64_t cap, int64_t* m) {
        return mi_icp_stsdf_extract_point_cloud(Engine(), v, p, n, c, cap, m);
    });
}

std::shared_ptr<geometry::PointCloud> ScalableTSDFVolume::ExtractVoxelPointCloud() {
    mi_icp_stsdf* v = volume_;
    return FillCloud(false, true, kFirstCapacity, [v](float* p, float*, float* c, int64_t cap, int64_t* m) {
        return mi_icp_stsdf_extract_voxel_point_cloud(Engine(), v, p, c, cap, m);
    });
}

size_t ScalableTSDFVolume::NumVolumeUnits() const {
    int64_t n = 0;
    Check(mi_icp_stsdf_num_units(Engine(), volume_, &n, nullptr));
    return (size_t)n;
}

std::vector<ScalableTSDFVolume::VolumeUnit> ScalableTSDFVolume::GetVolumeUnits() const {
    const size_t units = NumVolumeUnits(), n = units * 4096;
    const bool colored = color_type_ != TSDFVolumeColorType::NoColor;
    std::vector<VolumeUnit> none;
    if (units == 0) return none;
    // the read-back fills device arrays: keys [units][3], then tsdf, weight and colour planes as floats
    utility::device_vector<int32_t> dkeys(units * 3);
    utility::device_vector<float> dt(n), dw(n), dc(colored ? 3 * n : 0);
    int64_t m = 0;
    Check(mi_icp_stsdf_get_units(Engine(), volume_, dkeys.data(), dt.data(), dw.data(), colored ? dc.data() : nullptr,
                                 (int64_t)units, &m));
    const std::vector<int32_t> keys = dkeys.to_host();
    const std::vector<float> t = dt.to_host(), w = dw.to_host(), c = dc.to_host();
    std::vector<VolumeUnit> out(units);
    for (size_t e = 0; e < units; ++e) {
        out[e].index_ = Eigen::Vector3i(keys[e * 3], keys[e * 3 + 1], keys[e * 3 + 2]);
        out[e].voxels_.resize(4096);
        for (size_t v = 0; v < 4096; ++v) {
            const size_t i = e * 4096 + v;
            out[e].voxels_[v].tsdf_ = t[i];
            out[e].voxels_[v].weight_ = w[i];
            if (colored) out[e].voxels_[v].color_ = Eigen::Vector3f(c[i], c[n + i], c[2 * n + i]);
        }
    }
    return out;
}

}  // namespace integration

// ---------------------------------------------------------------- kinfu
namespace kinfu {

namespace {
template <class Level>
PointCloudPyramid CloudPyramid(const camera::PinholeCameraIntrinsic& intrinsic, const KinfuOption& option, Level level) {
    PointCloudPyramid out((size_t)option.num_pyramid_levels_);
    for (int i = 0; i < option.num_pyramid_levels_; ++i)
        out[(size_t)i] = geometry::PointCloud::CreateFromRGBDImage(level((size_t)i), intrinsic.CreatePyramidLevel((size_t)i),
                                                                   Eigen::Matrix4f::Identity(), true,
                                                                   option.depth_cutoff_, true);
    return out;
}
}  // namespace

PointCloudPyramid CreatePointCloudPyramid(const std::vector<geometry::RGBDImage>& image_pyramid,
                                          const camera::PinholeCameraIntrinsic& intrinsic,
                                          const KinfuOption& option) {
    return CloudPyramid(intrinsic, option, [&](size_t i) -> const geometry::RGBDImage& { return image_pyramid[i]; });
}

PointCloudPyramid CreatePointCloudPyramid(const geometry::RGBDImagePyramid& image_pyramid,
                                          const camera::PinholeCameraIntrinsic& intrinsic,
                                          const KinfuOption& option) {
    return CloudPyramid(intrinsic, option, [&](size_t i) -> const geometry::RGBDImage& { return *image_pyramid[i]; });
}

std::tuple<Eigen::Matrix4f, bool> PoseEstimation(const KinfuOption& option, const Eigen::Matrix4f& extrinsic,
                                                 const PointCloudPyramid& frame_data,
                                                 const PointCloudPyramid& target_data) {
    Eigen::Matrix4f cur = extrinsic;
    for (int level = option.num_pyramid_levels_ - 1; level >= 0; --level) {
        registration::ICPConvergenceCriteria criteria;
        criteria.max_iteration_ = option.icp_iterations_[(size_t)level];
        switch (option.tf_type_) {
            case registration::TransformationEstimationType::PointToPlane: {
                auto res = registration::RegistrationICP(*frame_data[(size_t)level], *target_data[(size_t)level],
                                                         option.distance_threshold_, cur,
                                                         registration::TransformationEstimationPointToPlane(100000),
                                                         criteria);
                cur = res.transformation_;
                break;
            }
            case registration::TransformationEstimationType::ColoredICP: {
                auto res = registration::RegistrationColoredICP(*frame_data[(size_t)level], *target_data[(size_t)level],
                                                                option.distance_threshold_, cur, criteria, 0.968f, 100000);
                cur = res.transformation_;
                break;
            }
            default:
                LogError("[KinfuPipeline::PoseEstimation] Unsupported transformation type.");
                break;
        }
    }
    return std::make_tuple(cur, true);
}

KinfuPipeline::KinfuPipeline(const camera::PinholeCameraIntrinsic& intrinsic, const KinfuOption& option)
    : intrinsic_(intrinsic),
      volume_(option.tsdf_length_, option.tsdf_resolution_, option.sdf_trunc_, option.tsdf_color_type_, option.tsdf_origin_),
      option_(option) {}

KinfuPipeline::~KinfuPipeline() {}

void KinfuPipeline::Reset() {
    cur_pose_ = Eigen::Matrix4f::Identity();
    volume_.Reset();
    model_pyramid_.clear();
    frame_id_ = 0;
}

bool KinfuPipeline::ProcessFrame(const geometry::RGBDImage& image) {
    const auto refuse = [](const char* why) {
        LogError((std::string("[KinfuPipeline::ProcessFrame] ") + why).c_str());
        return false;
    };
    const int levels = option_.num_pyramid_levels_;
    if (!image.color_.HasData() || !image.depth_.HasData()) return refuse("The frame has no colour or no depth data.");
    if (levels < 1 || levels > kMaxPyramidLevels) return refuse("num_pyramid_levels must be in [1, 16].");
    if (option_.icp_iterations_.size() < (size_t)levels) return refuse("icp_iterations has fewer entries than num_pyramid_levels.");
    if (image.color_.width_ != intrinsic_.width_ || image.color_.height_ != intrinsic_.height_ ||
        image.depth_.width_ != intrinsic_.width_ || image.depth_.height_ != intrinsic_.height_)
        return refuse("The frame's size is not the intrinsic's.");
    // SurfaceMeasurement (kinfu.cpp:86-104)
    const geometry::RGBDImagePyramid pyramid = image.CreatePyramid((size_t)levels);
    if (pyramid.size() != (size_t)levels) return refuse("Unsupported image format.");
    const geometry::RGBDImagePyramid smooth =
            geometry::RGBDImage::BilateralFilterPyramidDepth(pyramid, option_.diameter_, option_.sigma_depth_, option_.sigma_space_);
    const PointCloudPyramid pc_pyramid = CreatePointCloudPyramid(smooth, intrinsic_, option_);
    Eigen::Matrix4f extrinsic = utility::InverseTransform(cur_pose_);
    if (frame_id_ > 0) extrinsic = std::get<0>(PoseEstimation(option_, extrinsic, model_pyramid_, pc_pyramid));
    // the volume turns a format away before it changes anything: the pose is kept only with an integrated frame
    if (!volume_.TryIntegrate(*smooth[0], intrinsic_, extrinsic)) return refuse("Unsupported image format.");
    if (frame_id_ > 0) cur_pose_ = utility::InverseTransform(extrinsic);
    model_pyramid_ = volume_.RaycastLevels(intrinsic_, extrinsic, option_.sdf_trunc_, levels);
    frame_id_++;
    return true;
}

std::shared_ptr<geometry::PointCloud> KinfuPipeline::ExtractPointCloud() { return volume_.ExtractPointCloud(); }

}  // namespace kinfu

// ---------------------------------------------------------------- geometry::LaserScanBuffer (laserscanbuffer.cu, laserscanbuffer_factory.cu) over mi_icp_laserscan_*
namespace geometry {

namespace {
// a*b, every element ((a0*b0 + a1*b1) + a2*b2) + a3*b3 (include/mi_icp.h "laserscan")
Eigen::Matrix4f Mul4(const Eigen::Matrix4f& a, const Eigen::Matrix4f& b) {
    Eigen::Matrix4f out;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out(r, c) = ((a(r, 0) * b(0, c) + a(r, 1) * b(1, c)) + a(r, 2) * b(2, c)) + a(r, 3) * b(3, c);
    return out;
}

Eigen::Matrix4f QuarterTurnX() {  // the exact -pi/2 about X: rows (1,0,0), (0,0,1), (0,-1,0)
    Eigen::Matrix4f q = Eigen::Matrix4f::Identity();
    q(1, 1) = 0.0f;
    q(1, 2) = 1.0f;
    q(2, 1) = -1.0f;
    q(2, 2) = 0.0f;
    return q;
}

void MakeStorage(LaserScanBuffer* b, bool with_intensities) {
    const size_t count = (size_t)b->num_max_scans_ * (size_t)b->num_steps_;
    if (b->ranges_.size() != count) {
        b->ranges_ = std::vector<float>(count, std::numeric_limits<float>::quiet_NaN());
    }
    if (with_intensities && b->intensities_.size() != count) b->intensities_ = std::vector<float>(count, 0.0f);
}

// one scan into the ring; `device`: where ranges / intensities live
LaserScanBuffer& AddScan(LaserScanBuffer* b, const float* ranges, size_t n, const Eigen::Matrix4f& transformation,
                         const float* intensities, size_t ni, bool device) {
    if ((int)n != b->num_steps_ || b->num_max_scans_ < 1) {
        LogError("[AddRanges] Invalid size of input ranges.");
        return *b;
    }
    if (b->HasIntensities() && n != ni) {
        LogError("[AddRanges] Invalid size of intensities.");
        return *b;
    }
    const bool first_with = b->IsEmpty() && !b->HasIntensities() && ni == n;
    MakeStorage(b, first_with);
    if (b->IsFull()) b->top_++;
    const size_t slot = (size_t)(b->bottom_ % b->num_max_scans_), bytes = n * sizeof(float);
    auto put = device ? utility::copy_d2d : utility::copy_h2d;
    put(b->ranges_.data() + slot * n, ranges, bytes);
    if (b->HasIntensities()) put(b->intensities_.data() + slot * n, intensities, bytes);
    b->origins_[slot] = transformation;
    b->bottom_++;
    return *b;
}

std::vector<float> Live(const LaserScanBuffer& b, const utility::device_vector<float>& store) {
    std::vector<float> out;
    if (store.empty()) return out;
    const size_t n = (size_t)b.num_steps_;
    out.resize((size_t)b.GetNumScans() * n);
    for (int k = 0; k < b.GetNumScans(); ++k)
        utility::copy_d2h(out.data() + (size_t)k * n, store.data() + (size_t)((b.top_ + k) % b.num_max_scans_) * n, n * sizeof(float));
    return out;
}

bool FactoryCheck(const char* what, const char* low_name, const char* high_name, float angle_increment, float low, float high,
                  float min_range, float max_range, float min_angle, float max_angle) {
    std::string msg;
    if (!(angle_increment > 0.0f)) msg = "angle_increment must be positive.";
    else if (!(low < high)) msg = std::string(low_name) + " must be smaller than " + high_name + ".";
    else if (!(min_range < max_range)) msg = "min_range must be smaller than max_range.";
    else if (!(min_angle < max_angle)) msg = "min_angle must be smaller than max_angle.";
    if (msg.empty()) return true;
    LogError((std::string("[LaserScanBuffer::") + what + "] " + msg).c_str());
    return false;
}

// the factories' buffer: max(DEFAULT_NUM_MAX_SCANS, divisions) NaN slots with their origins, `divisions` of them live
std::shared_ptr<LaserScanBuffer> FactoryBuffer(float angle_increment, float low, float high, unsigned int divisions, float min_angle,
                                               float max_angle, const Eigen::Matrix4f* left) {
    const float q = std::ceil((max_angle - min_angle) / angle_increment);
    int64_t lds = 0, most = 0;
    mi_icp_laserscan_limits(&lds, &most);
    if (!(q >= 1.0f && q <= (float)most) || divisions < 1 || (double)q * divisions > (double)most) {
        LogError("[LaserScanBuffer] too many bins, or none.");
        return nullptr;
    }
    auto out = std::make_shared<LaserScanBuffer>((int)q, (int)std::max(DEFAULT_NUM_MAX_SCANS, divisions), min_angle, max_angle);
    MakeStorage(out.get(), false);
    for (int i = 0; i < out->num_max_scans_; ++i) {
        Eigen::Matrix4f o = Eigen::Matrix4f::Identity();
        o(2, 3) = low + ((high - low) * (float)i) / (float)divisions;
        out->origins_[(size_t)i] = left ? Mul4(*left, o) : o;
    }
    out->bottom_ = (int)divisions;
    return out;
}
}  // namespace

LaserScanBuffer::LaserScanBuffer(int num_steps, int num_max_scans, float min_angle, float max_angle)
    : GeometryBase3D(GeometryType::LaserScanBuffer),
      num_steps_(num_steps),
      num_max_scans_(num_max_scans),
      min_angle_(min_angle),
      max_angle_(max_angle),
      origins_((size_t)std::max(num_max_scans, 0), Eigen::Matrix4f::Identity()) {}
LaserScanBuffer::~LaserScanBuffer() {}
LaserScanBuffer::LaserScanBuffer(const LaserScanBuffer& other)
    : GeometryBase3D(GeometryType::LaserScanBuffer),
      ranges_(other.ranges_),
      intensities_(other.intensities_),
      top_(other.top_),
      bottom_(other.bottom_),
      num_steps_(other.num_steps_),
      num_max_scans_(other.num_max_scans_),
      min_angle_(other.min_angle_),
      max_angle_(other.max_angle_),
      origins_(other.origins_) {}

thrust::host_vector<float> LaserScanBuffer::GetRanges() const { return Live(*this, ranges_); }
thrust::host_vector<float> LaserScanBuffer::GetIntensities() const { return Live(*this, intensities_); }

LaserScanBuffer& LaserScanBuffer::Clear() {
    top_ = bottom_ = 0;
    ranges_ = utility::device_vector<float>();
    intensities_ = utility::device_vector<float>();
    std::fill(origins_.begin(), origins_.end(), Eigen::Matrix4f::Identity());
    return *this;
}
bool LaserScanBuffer::IsEmpty() const { return bottom_ == top_; }

Eigen::Vector3f LaserScanBuffer::GetMinBound() const {
    LogError("LaserScanBuffer::GetMinBound is not supported");
    return Eigen::Vector3f::Zero();
}
Eigen::Vector3f LaserScanBuffer::GetMaxBound() const {
    LogError("LaserScanBuffer::GetMaxBound is not supported");
    return Eigen::Vector3f::Zero();
}
Eigen::Vector3f LaserScanBuffer::GetCenter() const {
    LogError("LaserScanBuffer::GetCenter is not supported");
    return Eigen::Vector3f::Zero();
}
AxisAlignedBoundingBox<3> LaserScanBuffer::GetAxisAlignedBoundingBox() const {
    LogError("LaserScanBuffer::GetAxisAlignedBoundingBox is not supported");
    return AxisAlignedBoundingBox<3>();
}

LaserScanBuffer& LaserScanBuffer::Transform(const Eigen::Matrix4f& transformation) {
    for (auto& o : origins_) o = Mul4(o, transformation);
    return *this;
}
LaserScanBuffer& LaserScanBuffer::Translate(const Eigen::Vector3f& translation, bool) {
    for (auto& o : origins_)
        for (int r = 0; r < 3; ++r) o(r, 3) = o(r, 3) + translation(r);
    return *this;
}
LaserScanBuffer& LaserScanBuffer::Scale(const float scale, bool) {
    Check(mi_icp_laserscan_scale(Engine(), ranges_.data(), (int64_t)ranges_.size(), scale));
    return *this;
}
LaserScanBuffer& LaserScanBuffer::Rotate(const Eigen::Matrix3f& R, bool) {
    for (auto& o : origins_) {
        const Eigen::Matrix4f a = o;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) o(r, c) = (a(r, 0) * R(0, c) + a(r, 1) * R(1, c)) + a(r, 2) * R(2, c);
    }
    return *this;
}

LaserScanBuffer& LaserScanBuffer::AddRanges(const utility::device_vector<float>& ranges, const Eigen::Matrix4f& transformation,
                                            const utility::device_vector<float>& intensities) {
    return AddScan(this, ranges.data(), ranges.size(), transformation, intensities.data(), intensities.size(), true);
}
LaserScanBuffer& LaserScanBuffer::AddRanges(const thrust::host_vector<float>& ranges, const Eigen::Matrix4f& transformation,
                                            const thrust::host_vector<float>& intensities) {
    return AddScan(this, ranges.data(), ranges.size(), transformation, intensities.data(), intensities.size(), false);
}
LaserScanBuffer& LaserScanBuffer::AddRanges(const float* ranges, const Eigen::Matrix4f& transformation, const float* intensities) {
    return AddScan(this, ranges, ranges ? (size_t)num_steps_ : 0, transformation, intensities, intensities ? (size_t)num_steps_ : 0, false);
}

LaserScanBuffer& LaserScanBuffer::Merge(const LaserScanBuffer& other) {
    if (other.IsEmpty()) {
        LogError("[Merge] Input buffer is empty.");
        return *this;
    }
    if (other.num_steps_ != num_steps_) {
        LogError("[Merge] Input buffer has different num_steps.");
        return *this;
    }
    if (other.HasIntensities() != HasIntensities()) {
        LogError("[Merge] Input buffer has different intensities.");
        return *this;
    }
    if (other.min_angle_ != min_angle_ || other.max_angle_ != max_angle_) {
        LogError("[Merge] Input buffer has different angle range.");
        return *this;
    }
    if (other.bottom_ - other.top_ + bottom_ - top_ > num_max_scans_) {
        LogError("[Merge] Buffer is full.");
        return *this;
    }
    const size_t n = (size_t)num_steps_;
    for (int k = 0; k < other.GetNumScans(); ++k) {
        const size_t slot = (size_t)((other.top_ + k) % other.num_max_scans_);
        AddScan(this, other.ranges_.data() + slot * n, n, other.origins_[slot],
                other.HasIntensities() ? other.intensities_.data() + slot * n : nullptr, other.HasIntensities() ? n : 0, true);
    }
    return *this;
}

std::shared_ptr<LaserScanBuffer> LaserScanBuffer::PopOneScan() {
    if (IsEmpty()) {
        LogError("[PopRange] Buffer is empty.");
        return nullptr;
    }
    const size_t slot = (size_t)(top_ % num_max_scans_), n = (size_t)num_steps_;
    auto out = std::make_shared<LaserScanBuffer>(num_steps_, num_max_scans_, min_angle_, max_angle_);
    AddScan(out.get(), ranges_.data() + slot * n, n, origins_[slot], HasIntensities() ? intensities_.data() + slot * n : nullptr,
            HasIntensities() ? n : 0, true);
    top_++;
    return out;
}

std::pair<std::unique_ptr<utility::pinned_host_vector<float>>, std::unique_ptr<utility::pinned_host_vector<float>>>
LaserScanBuffer::PopHostOneScan() {
    auto r = std::make_unique<utility::pinned_host_vector<float>>();
    auto v = std::make_unique<utility::pinned_host_vector<float>>();
    if (IsEmpty()) {
        LogError("[PopRange] Buffer is empty.");
        return std::make_pair(std::move(r), std::move(v));
    }
    const size_t slot = (size_t)(top_ % num_max_scans_), n = (size_t)num_steps_;
    r->resize(n);
    utility::copy_d2h(r->data(), ranges_.data() + slot * n, n * sizeof(float));
    if (HasIntensities()) {
        v->resize(n);
        utility::copy_d2h(v->data(), intensities_.data() + slot * n, n * sizeof(float));
    }
    top_++;
    return std::make_pair(std::move(r), std::move(v));
}

std::shared_ptr<LaserScanBuffer> LaserScanBuffer::RangeFilter(float min_range, float max_range) const {
    auto out = std::make_shared<LaserScanBuffer>(*this);
    if (max_range <= min_range) LogError("[RangeFilter] Invalid parameter with min_range greater than max_range.");
    Check(mi_icp_laserscan_range_filter(Engine(), ranges_.data(), (int64_t)ranges_.size(), min_range, max_range, out->ranges_.data()));
    return out;
}

std::shared_ptr<LaserScanBuffer> LaserScanBuffer::ScanShadowsFilter(float min_angle, float max_angle, int window, int neighbors,
                                                                    bool remove_shadow_start_point) const {
    auto out = std::make_shared<LaserScanBuffer>(*this);
    if (ranges_.empty()) return out;
    Check(mi_icp_laserscan_shadow_filter(Engine(), ranges_.data(), num_steps_, num_max_scans_, min_angle_, max_angle_, min_angle,
                                         max_angle, window, neighbors, remove_shadow_start_point ? 1 : 0, out->ranges_.data()));
    return out;
}

std::shared_ptr<LaserScanBuffer> LaserScanBuffer::CreateFromPointCloud(const geometry::PointCloud& pcd, float angle_increment,
                                                                       float min_height, float max_height,
                                                                       unsigned int num_vertical_divisions, float min_range,
                                                                       float max_range, float min_angle, float max_angle) {
    if (!FactoryCheck("CreateFromPointCloud", "min_height", "max_height", angle_increment, min_height, max_height, min_range,
                      max_range, min_angle, max_angle))
        return nullptr;
    auto out = FactoryBuffer(angle_increment, min_height, max_height, num_vertical_divisions, min_angle, max_angle, nullptr);
    if (!out) return nullptr;
    Check(mi_icp_laserscan_from_points(Engine(), Ptr(pcd.points_), (int64_t)pcd.points_.size(), angle_increment, min_height, max_height,
                                       (int32_t)num_vertical_divisions, min_range, max_range, min_angle, max_angle, out->num_steps_,
                                       out->ranges_.data(), nullptr));
    return out;
}

std::shared_ptr<LaserScanBuffer> LaserScanBuffer::CreateFromDepthImage(const geometry::Image& depth,
                                                                       const camera::PinholeCameraIntrinsic& intrinsic,
                                                                       float angle_increment, float min_y, float max_y,
                                                                       unsigned int num_vertical_divisions, float min_range,
                                                                       float max_range, float min_angle, float max_angle,
                                                                       float depth_scale, float depth_trunc, int stride) {
    if (!FactoryCheck("CreateFromDepthImage", "min_y", "max_y", angle_increment, min_y, max_y, min_range, max_range, min_angle,
                      max_angle))
        return nullptr;
    if (depth.num_of_channels_ != 1 || (depth.bytes_per_channel_ != 2 && depth.bytes_per_channel_ != 4) || stride < 1) {
        LogError("[LaserScanBuffer::CreateFromDepthImage] Unsupported image format.");
        return nullptr;
    }
    const Eigen::Matrix4f q = QuarterTurnX();
    auto out = FactoryBuffer(angle_increment, min_y, max_y, num_vertical_divisions, min_angle, max_angle, &q);
    if (!out) return nullptr;
    const float k4[4] = {intrinsic.fx_, intrinsic.fy_, intrinsic.cx_, intrinsic.cy_};
    Check(mi_icp_laserscan_from_depth(Engine(), depth.data_.data(), depth.bytes_per_channel_ == 2 ? MI_ICP_DEPTH_U16 : MI_ICP_DEPTH_F32,
                                      depth.width_, depth.height_, k4, depth_scale, depth_trunc, stride, angle_increment, min_y, max_y,
                                      (int32_t)num_vertical_divisions, min_range, max_range, min_angle, max_angle, out->num_steps_,
                                      out->ranges_.data(), nullptr));
    return out;
}

std::shared_ptr<PointCloud> PointCloud::CreateFromLaserScanBuffer(const LaserScanBuffer& scan, float min_range, float max_range) {
    auto out = std::make_shared<PointCloud>();
    if (scan.ranges_.size() == 0 || scan.IsEmpty()) {
        LogError("[PointCloud::CreateFromLaserScanBuffer] Empty scan, return empty pointcloud.");
        return out;
    }
    if (min_range >= max_range) {
        LogError("[PointCloud::CreateFromLaserScanBuffer] min_range must be smaller than max_range.");
        return out;
    }
    const size_t room = (size_t)scan.GetNumScans() * (size_t)scan.num_steps_;
    out->points_.resize(room);
    if (scan.HasIntensities()) out->colors_.resize(room);
    int64_t m = 0;
    Check(mi_icp_laserscan_to_points(Engine(), scan.ranges_.data(), scan.HasIntensities() ? scan.intensities_.data() : nullptr,
                                     scan.origins_.data()->data(), scan.num_steps_, scan.num_max_scans_, scan.top_ % scan.num_max_scans_,
                                     scan.GetNumScans(), scan.min_angle_, scan.max_angle_, min_range, max_range,
                                     out->points_.data()->data(), scan.HasIntensities() ? out->colors_.data()->data() : nullptr,
                                     (int64_t)room, &m));
    out->points_.resize((size_t)m);
    if (scan.HasIntensities()) out->colors_.resize((size_t)m);
    return out;
}

}  // namespace geometry

// ---------------------------------------------------------------- geometry::Image / RGBDImage processing
// (geometry/image.cu, image_factory.cu, rgbdimage.cu, rgbdimage_factory.cu over mi_icp_image_*)
namespace geometry {

namespace {

bool IsFormat(const Image& im, int channels, int bytes) { return im.num_of_channels_ == channels && im.bytes_per_channel_ == bytes; }

bool KnownFormat(const Image& im) {
    return im.num_of_channels_ >= 1 && im.num_of_channels_ <= 4 && (im.bytes_per_channel_ == 1 || im.bytes_per_channel_ == 2 || im.bytes_per_channel_ == 4);
}

void FilterTaps(Image::FilterType type, std::vector<float>* dx, std::vector<float>* dy) {
    const std::vector<float> s1 = {-1.0f, 0.0f, 1.0f}, s2 = {1.0f, 2.0f, 1.0f};
    switch (type) {
        case Image::FilterType::Gaussian3: *dx = *dy = {0.25f, 0.5f, 0.25f}; break;
        case Image::FilterType::Gaussian5: *dx = *dy = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}; break;
        case Image::FilterType::Gaussian7: *dx = *dy = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}; break;
        case Image::FilterType::Sobel3Dx: *dx = s1; *dy = s2; break;
        case Image::FilterType::Sobel3Dy: *dx = s2; *dy = s1; break;
        default: dx->clear(); dy->clear(); break;
    }
}

bool GoodTaps(const std::vector<float>& k) { return k.size() % 2 == 1 && k.size() <= (size_t)MI_ICP_IMAGE_MAX_TAPS; }

std::shared_ptr<Image> Move(const Image& im, int op, const char* error) {
    auto out = std::make_shared<Image>();
    if (im.IsEmpty()) return out;
    if (!KnownFormat(im)) {
        LogError(error);
        return out;
    }
    if (op == MI_ICP_IMAGE_TRANSPOSE) out->Prepare(im.height_, im.width_, im.num_of_channels_, im.bytes_per_channel_);
    else out->Prepare(im.width_, im.height_, im.num_of_channels_, im.bytes_per_channel_);
    Check(mi_icp_image_move(Engine(), im.data_.data(), im.width_, im.height_, im.num_of_channels_ * im.bytes_per_channel_, op, out->data_.data()));
    return out;
}

// one format factory: the depth decoded (format >= 0), then CreateFromColorAndDepth
std::shared_ptr<RGBDImage> FromFormat(const Image& color, const Image& depth, int format, const char* error, float scale, float trunc,
                                      bool convert_rgb_to_intensity) {
    if (color.height_ != depth.height_ || color.width_ != depth.width_ || !IsFormat(depth, 1, 2)) {
        LogError(error);
        return std::make_shared<RGBDImage>();
    }
    Image decoded = depth;
    if (!depth.IsEmpty())
        Check(mi_icp_image_depth_format(Engine(), (const uint16_t*)depth.data_.data(), depth.width_, depth.height_, format, (uint16_t*)decoded.data_.data()));
    return RGBDImage::CreateFromColorAndDepth(color, decoded, scale, trunc, convert_rgb_to_intensity);
}

}  // namespace

std::shared_ptr<Image> Image::ConvertDepthToFloatImage(float depth_scale, float depth_trunc) const {
    auto out = std::make_shared<Image>();
    if (IsEmpty()) return out;
    if (!KnownFormat(*this)) {
        LogError("[ConvertDepthToFloatImage] Unsupported image format.");
        return out;
    }
    out->Prepare(width_, height_, 1, 4);
    Check(mi_icp_image_depth_to_float(Engine(), data_.data(), width_, height_, num_of_channels_, bytes_per_channel_, depth_scale, depth_trunc,
                                      (float*)out->data_.data()));
    return out;
}

std::shared_ptr<Image> Image::Transpose() const { return Move(*this, MI_ICP_IMAGE_TRANSPOSE, "[Transpose] Unsupported image format."); }
std::shared_ptr<Image> Image::FlipHorizontal() const { return Move(*this, MI_ICP_IMAGE_FLIP_HORIZONTAL, "[FlipHorizontal] Unsupported image format."); }
std::shared_ptr<Image> Image::FlipVertical() const { return Move(*this, MI_ICP_IMAGE_FLIP_VERTICAL, "[FlipVertical] Unsupported image format."); }

std::shared_ptr<Image> Image::FilterHorizontal(const std::vector<float>& kernel) const {
    auto out = std::make_shared<Image>();
    if (IsEmpty() || !IsFormat(*this, 1, 4) || !GoodTaps(kernel)) {
        LogError("[FilterHorizontal] Unsupported image format or kernel size.");
        return out;
    }
    out->Prepare(width_, height_, 1, 4);
    Check(mi_icp_image_filter(Engine(), (const float*)data_.data(), width_, height_, kernel.data(), (int)kernel.size(), nullptr, 0,
                              (float*)out->data_.data()));
    return out;
}

std::shared_ptr<Image> Image::Filter(const std::vector<float>& dx, const std::vector<float>& dy) const {
    auto out = std::make_shared<Image>();
    if (IsEmpty() || !IsFormat(*this, 1, 4)) {
        LogError("[Filter] Unsupported image format.");
        return out;
    }
    if (!GoodTaps(dx) || !GoodTaps(dy)) {
        LogError("[FilterHorizontal] Unsupported image format or kernel size.");
        return out;
    }
    out->Prepare(width_, height_, 1, 4);
    Check(mi_icp_image_filter(Engine(), (const float*)data_.data(), width_, height_, dx.data(), (int)dx.size(), dy.data(), (int)dy.size(),
                              (float*)out->data_.data()));
    return out;
}

std::shared_ptr<Image> Image::Filter(FilterType type) const {
    std::vector<float> dx, dy;
    FilterTaps(type, &dx, &dy);
    if (dx.empty()) {
        LogError("[Filter] Unsupported filter type.");
        return std::make_shared<Image>();
    }
    return Filter(dx, dy);
}

std::shared_ptr<Image> Image::Downsample() const {
    auto out = std::make_shared<Image>();
    if (IsEmpty() || (!IsFormat(*this, 1, 4) && !IsFormat(*this, 3, 1))) {
        LogError("[Downsample] Unsupported image format.");
        return out;
    }
    if (width_ / 2 == 0 || height_ / 2 == 0) return out;
    out->Prepare(width_ / 2, height_ / 2, num_of_channels_, bytes_per_channel_);
    Check(mi_icp_image_downsample(Engine(), data_.data(), width_, height_, num_of_channels_, bytes_per_channel_, out->data_.data()));
    return out;
}

std::shared_ptr<Image> Image::BilateralFilter(int diameter, float sigma_color, float sigma_space) const {
    auto out = std::make_shared<Image>();
    if (diameter < 0 || diameter > MI_ICP_IMAGE_MAX_DIAMETER) {
        LogError("[BilateralFilter] Diameter should be in [0, 31].");
        return out;
    }
    if (IsEmpty() || !IsFormat(*this, 1, 4)) {
        LogError("[BilateralFilter] Unsupported image format.");
        return out;
    }
    float table[2 * MI_ICP_IMAGE_MAX_DIAMETER + 1];
    Check(mi_icp_image_bilateral_table(diameter, sigma_space, table));
    out->Prepare(width_, height_, 1, 4);
    Check(mi_icp_image_bilateral(Engine(), (const float*)data_.data(), width_, height_, diameter, sigma_color, table, (float*)out->data_.data()));
    return out;
}

Image& Image::ClipIntensity(float min, float max) {
    if (IsEmpty() || !IsFormat(*this, 1, 4)) {
        LogError("[ClipIntensity] Unsupported image format.");
        return *this;
    }
    Check(mi_icp_image_clip(Engine(), (float*)data_.data(), width_, height_, min, max));
    return *this;
}

Image& Image::LinearTransform(float scale, float offset) {
    if (IsEmpty() || !KnownFormat(*this) || (bytes_per_channel_ != 1 && !IsFormat(*this, 1, 4))) {
        LogError("[LinearTransform] Unsupported image format.");
        return *this;
    }
    Check(mi_icp_image_linear_transform(Engine(), data_.data(), width_, height_, num_of_channels_, bytes_per_channel_, scale, offset));
    return *this;
}

std::shared_ptr<Image> Image::CreateGrayImage(ColorToIntensityConversionType type) const {
    auto out = std::make_shared<Image>();
    if (IsEmpty()) return out;
    if (!KnownFormat(*this)) {
        LogError("[CreateGrayImage] Unsupported image format.");
        return out;
    }
    out->Prepare(width_, height_, 1, 1);
    Check(mi_icp_image_create_gray(Engine(), data_.data(), width_, height_, num_of_channels_, bytes_per_channel_, (int)type, out->data_.data()));
    return out;
}

std::shared_ptr<Image> Image::CreateFloatImage(ColorToIntensityConversionType type) const {
    auto out = std::make_shared<Image>();
    if (IsEmpty()) return out;
    if (!KnownFormat(*this)) {
        LogError("[CreateFloatImage] Unsupported image format.");
        return out;
    }
    out->Prepare(width_, height_, 1, 4);
    Check(mi_icp_image_create_float(Engine(), data_.data(), width_, height_, num_of_channels_, bytes_per_channel_, (int)type,
                                    (float*)out->data_.data()));
    return out;
}

template <typename T>
std::shared_ptr<Image> Image::CreateImageFromFloatImage() const {
    auto out = std::make_shared<Image>();
    if (IsEmpty() || !IsFormat(*this, 1, 4)) {
        LogError("[CreateImageFromFloatImage] Unsupported image format.");
        return out;
    }
    out->Prepare(width_, height_, 1, (int)sizeof(T));
    Check(mi_icp_image_from_float(Engine(), (const float*)data_.data(), width_, height_, (int)sizeof(T), out->data_.data()));
    return out;
}
template std::shared_ptr<Image> Image::CreateImageFromFloatImage<uint8_t>() const;
template std::shared_ptr<Image> Image::CreateImageFromFloatImage<uint16_t>() const;

ImagePyramid Image::CreatePyramid(size_t num_of_levels, bool with_gaussian_filter) const {
    ImagePyramid pyramid;
    if (IsEmpty() || (!IsFormat(*this, 1, 4) && !IsFormat(*this, 3, 1))) {
        LogError("[CreateImagePyramid] Unsupported image format.");
        return pyramid;
    }
    for (size_t i = 0; i < num_of_levels; ++i) {
        if (i == 0) {
            pyramid.emplace_back(std::make_shared<Image>(*this));
            continue;
        }
        const Image& prev = *pyramid[i - 1];
        auto level = std::make_shared<Image>();
        if (prev.width_ / 2 > 0 && prev.height_ / 2 > 0) {
            if (with_gaussian_filter && num_of_channels_ == 1) {   // Downsample(Filter(Gaussian3)) in one kernel
                level->Prepare(prev.width_ / 2, prev.height_ / 2, 1, 4);
                Check(mi_icp_image_pyramid_level(Engine(), (const float*)prev.data_.data(), prev.width_, prev.height_, (float*)level->data_.data()));
            } else {
                level = prev.Downsample();
            }
        }
        pyramid.emplace_back(level);
    }
    return pyramid;
}

ImagePyramid Image::FilterPyramid(const ImagePyramid& input, FilterType type) {
    ImagePyramid out;
    for (const auto& level : input) out.emplace_back(level->Filter(type));
    return out;
}

ImagePyramid Image::BilateralFilterPyramid(const ImagePyramid& input, int diameter, float sigma_color, float sigma_space) {
    ImagePyramid out;
    for (const auto& level : input) out.emplace_back(level->BilateralFilter(diameter, sigma_color, sigma_space));
    return out;
}

std::shared_ptr<RGBDImage> RGBDImage::CreateFromColorAndDepth(const Image& color, const Image& depth, float depth_scale, float depth_trunc,
                                                              bool convert_rgb_to_intensity) {
    auto out = std::make_shared<RGBDImage>();
    if (color.height_ != depth.height_ || color.width_ != depth.width_) {
        LogError("[CreateFromColorAndDepth] Unsupported image format.");
        return out;
    }
    out->depth_ = *depth.ConvertDepthToFloatImage(depth_scale, depth_trunc);
    out->color_ = convert_rgb_to_intensity ? *color.CreateFloatImage() : color;
    return out;
}

std::shared_ptr<RGBDImage> RGBDImage::CreateFromRedwoodFormat(const Image& color, const Image& depth, bool convert_rgb_to_intensity) {
    return CreateFromColorAndDepth(color, depth, 1000.0f, 4.0f, convert_rgb_to_intensity);
}

std::shared_ptr<RGBDImage> RGBDImage::CreateFromTUMFormat(const Image& color, const Image& depth, bool convert_rgb_to_intensity) {
    return CreateFromColorAndDepth(color, depth, 5000.0f, 4.0f, convert_rgb_to_intensity);
}

std::shared_ptr<RGBDImage> RGBDImage::CreateFromSUNFormat(const Image& color, const Image& depth, bool convert_rgb_to_intensity) {
    return FromFormat(color, depth, MI_ICP_IMAGE_SUN, "[CreateRGBDImageFromSUNFormat] Unsupported image format.", 1000.0f, 7.0f, convert_rgb_to_intensity);
}

std::shared_ptr<RGBDImage> RGBDImage::CreateFromNYUFormat(const Image& color, const Image& depth, bool convert_rgb_to_intensity) {
    return FromFormat(color, depth, MI_ICP_IMAGE_NYU, "[CreateRGBDImageFromNYUFormat] Unsupported image format.", 1000.0f, 7.0f, convert_rgb_to_intensity);
}

RGBDImagePyramid RGBDImage::CreatePyramid(size_t num_of_levels, bool with_gaussian_filter_for_color, bool with_gaussian_filter_for_depth) const {
    RGBDImagePyramid out;
    const ImagePyramid color = color_.CreatePyramid(num_of_levels, with_gaussian_filter_for_color);
    const ImagePyramid depth = depth_.CreatePyramid(num_of_levels, with_gaussian_filter_for_depth);
    if (color.size() != num_of_levels || depth.size() != num_of_levels) return out;
    for (size_t i = 0; i < num_of_levels; ++i) out.emplace_back(std::make_shared<RGBDImage>(*color[i], *depth[i]));
    return out;
}

RGBDImagePyramid RGBDImage::FilterPyramid(const RGBDImagePyramid& rgbd_image_pyramid, Image::FilterType type) {
    RGBDImagePyramid out;
    for (const auto& level : rgbd_image_pyramid)
        out.emplace_back(std::make_shared<RGBDImage>(*level->color_.Filter(type), *level->depth_.Filter(type)));
    return out;
}

RGBDImagePyramid RGBDImage::BilateralFilterPyramidDepth(const RGBDImagePyramid& rgbd_image_pyramid, int diameter, float sigma_depth,
                                                        float sigma_space) {
    RGBDImagePyramid out;
    for (const auto& level : rgbd_image_pyramid)
        out.emplace_back(std::make_shared<RGBDImage>(level->color_, *level->depth_.BilateralFilter(diameter, sigma_depth, sigma_space)));
    return out;
}

}  // namespace geometry

}  // namespace cupoch
