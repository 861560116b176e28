// cupoch/registration/feature.h (reference: registration/feature.h): per-point descriptors as data.  The descriptor
// COMPUTATIONS (ComputeFPFHFeature, ComputeSHOTFeature) are not part of this library; a Feature is filled by its user.
#pragma once
#include <cstddef>

#include "cupoch/registration/transformation_estimation.h"
#include "cupoch/utility/device_vector.h"
#include "cupoch/utility/eigen.h"

namespace cupoch {
namespace registration {

template <int Dim>
class Feature {
public:
    typedef Eigen::Matrix<float, Dim, 1> FeatureType;
    void Resize(int n) { data_.resize(n < 0 ? 0 : (size_t)n); }
    size_t Dimension() const { return (size_t)Dim; }
    size_t Num() const { return data_.size(); }
    bool IsEmpty() const { return data_.empty(); }
    thrust::host_vector<FeatureType> GetData() const { return data_.to_host(); }
    void SetData(const thrust::host_vector<FeatureType>& data) { data_ = data; }

    utility::device_vector<FeatureType> data_;  // [Num()][Dim] floats, row after row
};

/// Row i = (i, nearest target feature of source feature i) for every source row that has one.  mutual_filter: only the
/// rows whose neighbour points back, unless fewer than mutual_consistency_ratio * n remain -- then the unfiltered list.
/// (The reference declares this function and defines it nowhere; include/mi_icp.h holds the definition used here.)
template <int Dim>
CorrespondenceSet CorrespondencesFromFeatures(const Feature<Dim>& source_features, const Feature<Dim>& target_features,
                                              bool mutual_filter = false, float mutual_consistency_ratio = 0.1f);

}  // namespace registration
}  // namespace cupoch
