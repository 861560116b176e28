"""cupoch.imageproc mirror (src/cupoch/imageproc/sgm.h; python surface src/python/cupoch_pybind/imageproc/imageproc.cpp):
SGMOption and SemiGlobalMatching.  The reference wraps libSGM, whose sources its checkout does not hold; what runs here
is this library's own semi-global matching in HIP, with the contract stated in include/mi_icp.h ("stereo") and DESIGN
4.13 and exactly SGMOption's parameters.  Images are geometry.Image, built from numpy or from a CUDA tensor; the result
is a geometry.Image whose pixels stay on the device."""
import enum

import numpy as np

from . import geometry
from ._lib import MI_ICP_ERR_INVALID, MiIcpError

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class DisparitySizeType(enum.IntEnum):
    DisparitySize64 = 64
    DisparitySize128 = 128
    DisparitySize256 = 256


class PathType(enum.IntEnum):
    ScanPath4 = 0
    ScanPath8 = 1


DisparitySize64, DisparitySize128, DisparitySize256 = DisparitySizeType     # exported values, as in the reference
ScanPath4, ScanPath8 = PathType


class SGMOption:
    """imageproc::SGMOption (sgm.h:30-70), the fields under the names of the reference's binding"""

    def __init__(self, width=0, height=0, p1=10, p2=120, uniqueness=0.95, disp_size=DisparitySizeType.DisparitySize128,
                 path_type=PathType.ScanPath8, min_disp=0, lr_max_diff=1):
        self.width = int(width)
        self.height = int(height)
        self.p1 = int(p1)
        self.p2 = int(p2)
        self.uniqueness = float(uniqueness)
        self.disp_size = disp_size
        self.path_type = path_type
        self.min_disp = int(min_disp)
        self.lr_max_diff = int(lr_max_diff)


def census(image):
    """the census words of a 1 x uint8 image (stage 1 of the contract) as an [H, W] int32 device tensor holding the
    unsigned words' bits (tests and measurements)"""
    image = image if isinstance(image, geometry.Image) else geometry.Image(image)
    if not image._is(1, 1):
        raise TypeError("census takes a 1 x uint8 image")
    eng, t = image._staged()
    return eng.sgm_census(t.reshape(image.height, image.width))


def _log_error(where, what):
    print("[cupoch_amd] Error: [SemiGlobalMatching::%s] %s" % (where, what))


class SemiGlobalMatching:
    """imageproc::SemiGlobalMatching (sgm.h:72-85).  The whole workspace is allocated here, for the option's size; an
    option the contract turns away is logged, and every process_frame then logs "Invalid SGM parameters." and returns
    an empty image, as the reference does for a zero size.  Not copyable."""

    def __init__(self, option, device=None):
        o = option
        self._size = (int(o.width), int(o.height))
        self._disp_size = int(o.disp_size)
        self._matcher = None
        self._eng = None
        if self._size[0] <= 0 or self._size[1] <= 0:       # before any engine: no device is needed to be turned away
            _log_error("SemiGlobalMatching", "Invalid SGM parameters: width and height must be positive.")
            return
        eng = geometry.get_engine(device)
        try:
            self._matcher = eng.sgm_create(o.width, o.height, o.p1, o.p2, o.uniqueness, int(o.disp_size), int(o.path_type),
                                           o.min_disp, o.lr_max_diff)
            self._eng = eng
        except MiIcpError as e:
            if e.code != MI_ICP_ERR_INVALID:
                raise
            _log_error("SemiGlobalMatching", "Invalid SGM parameters: %s" % e)

    def __copy__(self):
        raise TypeError("SemiGlobalMatching is not copyable")

    def __deepcopy__(self, memo):
        raise TypeError("SemiGlobalMatching is not copyable")

    def __del__(self):
        try:
            if self._matcher is not None:
                self._eng.sgm_destroy(self._matcher)
        except Exception:
            pass
        self._matcher = None

    def process_frame(self, left, right):
        left, right = (x if isinstance(x, geometry.Image) else geometry.Image(x) for x in (left, right))
        if self._matcher is None:
            _log_error("ProcessFrame", "Invalid SGM parameters.")
            return geometry.Image()
        if not (left._is(1, 1) and right._is(1, 1) and (left.width, left.height) == (right.width, right.height) == self._size):
            _log_error("ProcessFrame", "Unsupport image type.")
            return geometry.Image()
        if any(geometry._is_torch(x.data) and x.data.is_cuda and x.data.device.index != self._eng.device for x in (left, right)):
            raise MiIcpError("an image on another device than the matcher's")
        return geometry.Image(self._eng.sgm_process(self._matcher, self._on_device(left), self._on_device(right)))

    def _on_device(self, image):
        d = image.data.reshape(image.height, image.width)
        if geometry._is_torch(d) and d.is_cuda:
            return d.contiguous()
        a = d.detach().numpy() if geometry._is_torch(d) else np.asarray(d)
        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", self._eng.device))

    def get_sums(self):
        """S of the last frame, [H, W, D] uint16 on the device (tests and measurements)"""
        return self._eng.sgm_get_sums(self._matcher, self._size[0], self._size[1], self._disp_size)
