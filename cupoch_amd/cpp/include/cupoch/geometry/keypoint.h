// cupoch/geometry/keypoint.h -- geometry::keypoint (reference: geometry/keypoint.h): keypoint detectors on a
// PointCloud.  The operation runs HIP kernels through libmi_icp.so's C ABI (include/mi_icp.h states the contract).
#pragma once
#include <memory>
#include <tuple>

#include "cupoch/knn/kdtree_search_param.h"
#include "cupoch/utility/device_vector.h"

namespace cupoch {
namespace geometry {

class PointCloud;

namespace keypoint {

/// iss_keypoints.cu:108-172: Intrinsic Shape Signatures (Yu Zhong, 2009).  A point is a keypoint when the
/// eigenvalues e0 <= e1 <= e2 of the covariance of its neighbours within salient_radius (the nearest max_neighbors,
/// at least min_neighbors) have e1 / e2 < gamma_21 and e0 / e1 < gamma_32, and no point within non_max_radius has a
/// larger e0.  A radius of 0 has BOTH radii computed from the cloud's resolution (6 and 4 times it).  Returns the
/// keypoints (with normals and colours where the input has them) and one flag per input point.
/// max_neighbors must lie in [1, knn::NUM_MAX_NN]; anything else throws.
std::tuple<std::shared_ptr<PointCloud>, std::shared_ptr<utility::device_vector<bool>>> ComputeISSKeypoints(
        const PointCloud& input, float salient_radius = 0.0, float non_max_radius = 0.0, float gamma_21 = 0.975,
        float gamma_32 = 0.975, int min_neighbors = 5, int max_neighbors = knn::NUM_MAX_NN);

}  // namespace keypoint
}  // namespace geometry
}  // namespace cupoch
