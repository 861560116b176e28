// cupoch/camera/pinhole_camera_parameters.h -- camera::PinholeCameraParameters (reference:
// camera/pinhole_camera_parameters.h): an intrinsic and the world -> camera extrinsic, as the VoxelGrid carvings take
// them.  JSON conversion is not provided.
#pragma once
#include "cupoch/camera/pinhole_camera_intrinsic.h"

namespace cupoch {
namespace camera {

class PinholeCameraParameters {
public:
    PinholeCameraParameters() {}

public:
    PinholeCameraIntrinsic intrinsic_;
    Eigen::Matrix4f_u extrinsic_ = Eigen::Matrix4f_u::Identity();  // (the reference leaves it uninitialised)
};

}  // namespace camera
}  // namespace cupoch
