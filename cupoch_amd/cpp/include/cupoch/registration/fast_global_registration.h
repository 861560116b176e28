// cupoch/registration/fast_global_registration.h (reference: registration/fast_global_registration.h)
#pragma once
#include <cstdint>

#include "cupoch/geometry/pointcloud.h"
#include "cupoch/registration/feature.h"
#include "cupoch/registration/registration.h"

namespace cupoch {
namespace registration {

class FastGlobalRegistrationOption {
public:
    FastGlobalRegistrationOption(float division_factor = 1.4, bool use_absolute_scale = false, bool decrease_mu = true,
                                 float maximum_correspondence_distance = 0.025, int iteration_number = 64,
                                 float tuple_scale = 0.95, int maximum_tuple_count = 1000)
        : division_factor_(division_factor), use_absolute_scale_(use_absolute_scale), decrease_mu_(decrease_mu),
          maximum_correspondence_distance_(maximum_correspondence_distance), iteration_number_(iteration_number),
          tuple_scale_(tuple_scale), maximum_tuple_count_(maximum_tuple_count) {}
    float division_factor_;                  // par is divided by it every fourth iteration
    bool use_absolute_scale_;                // distances in the clouds' own unit, not relative to their extent
    bool decrease_mu_;                       // graduated non-convexity on / off
    float maximum_correspondence_distance_;  // where par stops shrinking; the result's inlier distance
    int iteration_number_;
    float tuple_scale_;                      // how alike a triple's side lengths must be
    int maximum_tuple_count_;                // correspondences kept from the tuple test
};

/// Instantiated for Dim = 33 and 352.  `seed` feeds the tuple draw: the same input and seed give the same bytes.
/// Empty inputs: an error is logged and a default RegistrationResult returned, as in the reference.
template <int Dim>
RegistrationResult FastGlobalRegistration(const geometry::PointCloud& source, const geometry::PointCloud& target,
                                          const Feature<Dim>& source_feature, const Feature<Dim>& target_feature,
                                          const FastGlobalRegistrationOption& option = FastGlobalRegistrationOption(),
                                          uint64_t seed = 0);

}  // namespace registration
}  // namespace cupoch
