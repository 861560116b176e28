"""imageproc and PointCloud.create_from_disparity of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp)
with the reference's Python names and defaults: names, enums and fields on the CPU, and on the GPU the bytes of the numpy
restatement (tests/sgm_exact.py) for one pair and one cloud.  Skips only where there is nothing to build the module with."""
import copy

import numpy as np
import pytest

import sgm_exact as sx

FIELDS = ("width", "height", "p1", "p2", "uniqueness", "disp_size", "path_type", "min_disp", "lr_max_diff")


def module():
    import importlib.util
    import shutil
    missing = [n for n in ("make", "g++") if shutil.which(n) is None] + ([] if importlib.util.find_spec("pybind11") else ["pybind11"])
    if missing:                 # nothing to build the module with: the only reason to skip
        pytest.skip("cupoch_pybind cannot be built here: no %s" % ", ".join(missing))
    from cupoch_amd import pybind as cph        # (a build or an import that breaks is a failure)
    return cph


def test_imageproc_has_the_references_names():
    cph = module()
    from cupoch_amd import imageproc as mirror
    for ip in (cph.imageproc, mirror):
        D, P = ip.DisparitySizeType, ip.PathType
        assert [int(D.DisparitySize64), int(D.DisparitySize128), int(D.DisparitySize256)] == [64, 128, 256]
        assert [int(P.ScanPath4), int(P.ScanPath8)] == [0, 1]
        assert ip.DisparitySize256 == D.DisparitySize256 and ip.ScanPath4 == P.ScanPath4      # exported values
        o = ip.SGMOption()
        assert [getattr(o, f) for f in FIELDS[:4]] == [0, 0, 10, 120] and o.uniqueness == pytest.approx(0.95)
        assert (o.disp_size, o.path_type, o.min_disp, o.lr_max_diff) == (D.DisparitySize128, P.ScanPath8, 0, 1)
        for f, v in zip(FIELDS, (64, 48, 7, 90, 0.9, D.DisparitySize64, P.ScanPath4, 2, -1)):
            setattr(o, f, v)                                                                   # read-write
            assert getattr(o, f) == (pytest.approx(v) if f == "uniqueness" else v)
        c = copy.copy(o)
        c.width = 5
        assert (o.width, c.width) == (64, 5)
        assert callable(ip.SemiGlobalMatching.process_frame)
    assert "baseline" in cph.geometry.PointCloud.create_from_disparity.__doc__
    assert "Factory function to create a pointcloud from a disparity image." in cph.geometry.PointCloud.create_from_disparity.__doc__
    from cupoch_amd import geometry
    assert callable(geometry.PointCloud.create_from_disparity)


@pytest.mark.gpu
def test_same_bytes_as_the_restatement(capfd):
    cph = module()
    ip, G = cph.imageproc, cph.geometry
    w, h = 130, 40
    left, right, _ = sx.pair(w, h, 3)
    o = ip.SGMOption()
    o.width, o.height = w, h
    sgm = ip.SemiGlobalMatching(o)
    disp = sgm.process_frame(G.Image(left), G.Image(right))
    want = sx.sgm(left, right)
    assert repr(disp) == "Image of size 130x40, with 1 channels."
    assert np.asarray(disp).tobytes() == want.tobytes() and (want != 255).mean() > 0.8
    color = np.random.default_rng(9).integers(0, 256, (h, w, 3)).astype(np.uint8)
    fx, fy, cx, cy, cxr, baseline = 517.3, 531.9, 64.6, 19.3, 61.25, 0.0754
    li, ri = cph.camera.PinholeCameraIntrinsic(w, h, fx, fy, cx, cy), cph.camera.PinholeCameraIntrinsic(w, h, fx, fy, cxr, cy)
    pc = G.PointCloud.create_from_disparity(disp, G.Image(color), li, ri, baseline)
    want_p, want_c = sx.points_from_disparity(want, color, fx, fy, cx, cy, cxr, baseline)
    assert sx.same_words(np.asarray(pc.points.cpu()), want_p) and sx.same_words(np.asarray(pc.colors.cpu()), want_c)
    # the error paths: a message and an empty result, nothing raised
    capfd.readouterr()
    assert ip.SemiGlobalMatching(ip.SGMOption()).process_frame(G.Image(left), G.Image(right)).is_empty()
    assert "Invalid SGM parameters." in capfd.readouterr().err
    assert sgm.process_frame(G.Image(left), G.Image(color)).is_empty()
    assert "Unsupport image type." in capfd.readouterr().err
    assert not G.PointCloud.create_from_disparity(G.Image(color), G.Image(color), li, ri, baseline).has_points()
    assert "[PointCloud::CreateFromDisparity] Unsupported image format." in capfd.readouterr().err
