// cupoch/knn/bruteforce_nn.h (reference: knn/bruteforce_nn.{h,inl}): the nearest `ref` row of every `query` row in
// feature space.  indices[i] = -1 and a NaN distance where every distance of row i is a NaN.  The distance is the
// squared one, summed as include/mi_icp.h states (mi_icp_feature_match); the ref x query matrix is never formed.
#pragma once
#include "cupoch/utility/device_vector.h"
#include "cupoch/utility/eigen.h"

namespace cupoch {
namespace knn {

template <int Dim>
void BruteForceNN(const utility::device_vector<Eigen::Matrix<float, Dim, 1>>& ref,
                  const utility::device_vector<Eigen::Matrix<float, Dim, 1>>& query, utility::device_vector<int>& indices,
                  utility::device_vector<float>& distances);

}  // namespace knn
}  // namespace cupoch
