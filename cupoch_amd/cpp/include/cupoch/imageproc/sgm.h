// cupoch/imageproc/sgm.h -- imageproc::SGMOption and imageproc::SemiGlobalMatching (reference: imageproc/sgm.h:30-85,
// sgm.cpp) over mi_icp_sgm_* (include/mi_icp.h "stereo" has the contract).  The reference wraps libSGM; this is the
// library's own semi-global matching with the same option members, enums and defaults: two rectified 1 x uint8 images
// in, one 1 x uint8 disparity image out.  The constructor allocates the whole workspace for the option's size.
#pragma once
#include <memory>

#include "cupoch/geometry/image.h"

struct mi_icp_sgm;

namespace cupoch {
namespace imageproc {

class SGMOption {
public:
    enum DisparitySizeType {
        DisparitySize64 = 64,
        DisparitySize128 = 128,
        DisparitySize256 = 256,
    };
    enum PathType {
        ScanPath4 = 0,
        ScanPath8 = 1,
    };

    SGMOption(int width = 0, int height = 0, int p1 = 10, int p2 = 120, float uniqueness = 0.95f,
              DisparitySizeType disp_size = DisparitySize128, PathType path_type = ScanPath8, int min_disp = 0,
              int lr_max_diff = 1)
        : width_(width),
          height_(height),
          p1_(p1),
          p2_(p2),
          uniqueness_(uniqueness),
          disp_size_(disp_size),
          path_type_(path_type),
          min_disp_(min_disp),
          lr_max_diff_(lr_max_diff) {}
    ~SGMOption() {}
    int width_;
    int height_;
    int p1_;
    int p2_;
    float uniqueness_;
    DisparitySizeType disp_size_;
    PathType path_type_;
    int min_disp_;
    int lr_max_diff_;
};

class SemiGlobalMatching {
public:
    /// An option the contract turns away (width or height not positive, not 0 <= p1 <= p2 <= 224, min_disp < 0 or
    /// min_disp + disp_size > 256) is logged; every ProcessFrame then logs "Invalid SGM parameters." and returns an
    /// empty image, as the reference does for a zero size.
    SemiGlobalMatching(const SGMOption& option);
    ~SemiGlobalMatching();
    SemiGlobalMatching(const SemiGlobalMatching&) = delete;
    SemiGlobalMatching& operator=(const SemiGlobalMatching&) = delete;
    /// Images of another size or format than width x height x 1 x uint8 log "Unsupport image type." and give an
    /// empty image.
    std::shared_ptr<geometry::Image> ProcessFrame(const geometry::Image& left, const geometry::Image& right);

public:
    const SGMOption option_;

private:
    mi_icp_sgm* matcher_ = nullptr;
};

}  // namespace imageproc
}  // namespace cupoch
