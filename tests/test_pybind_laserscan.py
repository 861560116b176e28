"""geometry.LaserScanBuffer of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp) with the
reference's Python names and defaults: names on the CPU, and on the GPU one round trip whose bytes equal the ctypes
mirror's.  Skips only where there is nothing to build the module with."""
import re

import numpy as np
import pytest

import laserscan_exact as lx

F = np.float32


def module():
    import importlib.util
    import shutil
    missing = [n for n in ("make", "g++") if shutil.which(n) is None] + ([] if importlib.util.find_spec("pybind11") else ["pybind11"])
    if missing:                 # nothing to build the module with: the only reason to skip
        pytest.skip("cupoch_pybind cannot be built here: no %s" % ", ".join(missing))
    from cupoch_amd import pybind as cph        # (a build or an import that breaks is a failure)
    return cph


def test_laserscan_rows_have_the_references_names():
    cph = module()
    L = cph.geometry.LaserScanBuffer
    for name in ("is_full", "add_ranges", "add_host_ranges", "merge", "pop_one_scan", "pop_host_one_scan", "range_filter",
                 "scan_shadow_filter", "create_from_point_cloud", "create_from_depth_image", "num_steps", "num_max_scans",
                 "min_angle", "max_angle", "num_scans", "ranges", "intensities"):
        assert hasattr(L, name), name
    assert hasattr(cph.geometry.PointCloud, "create_from_laserscanbuffer")

    def default(fn, name, value):            # "name: <the type, as this pybind11 spells it> = value"
        return re.search(r"\b%s: [^,)]*= %s[,)]" % (name, re.escape(value)), fn.__doc__) is not None
    assert default(L.__init__, "num_max_scans", "10")
    assert re.search(r"\bmin_angle: [^,)]*= -3\.14159\d*[,)]", L.__init__.__doc__)        # -pi, not the reference's +pi
    assert re.search(r"\bmax_angle: [^,)]*= 3\.14159\d*[,)]", L.__init__.__doc__)
    assert default(L.scan_shadow_filter, "neighbors", "0") and default(L.scan_shadow_filter, "remove_shadow_start_point", "False")
    assert default(L.create_from_point_cloud, "num_vertical_divisions", "1") and default(L.create_from_point_cloud, "max_range", "inf")
    assert default(L.create_from_depth_image, "depth_scale", "1000.0") and default(L.create_from_depth_image, "stride", "1")


@pytest.mark.gpu
def test_round_trip_equals_the_ctypes_mirror():
    cph = module()
    from cupoch_amd import geometry as g
    rng = np.random.default_rng(12)
    steps = 120
    a, b = cph.geometry.LaserScanBuffer(steps, 3, -2.0, 2.0), g.LaserScanBuffer(steps, 3, -2.0, 2.0)
    for k in range(4):                                       # wraps
        r = rng.uniform(0.5, 12.0, steps).astype(F)
        r[3 * k] = np.nan
        v = rng.random(steps).astype(F)
        T = lx.pose_matrix(0.3 * k, 1.0 - k, 0.2 * k, z=0.5)
        a.add_ranges(r, T, v)
        b.add_ranges(r, T, v)
    assert (a.num_scans, a.is_full(), a.num_steps, a.num_max_scans) == (3, True, steps, 3)
    assert np.asarray(a.ranges).tobytes() == b.get_ranges().tobytes()
    assert np.asarray(a.intensities).tobytes() == b.get_intensities().tobytes()
    fa, fb = a.range_filter(1.0, 9.0), b.range_filter(1.0, 9.0)
    assert np.asarray(fa.ranges).tobytes() == fb.get_ranges().tobytes() and np.isnan(fb.get_ranges()).sum() > 4
    sa, sb = fa.scan_shadow_filter(0.2, 2.9, 3, 1, True), fb.scan_shadow_filter(0.2, 2.9, 3, 1, True)
    assert np.asarray(sa.ranges).tobytes() == sb.get_ranges().tobytes()
    assert np.isnan(sb.get_ranges()).sum() > np.isnan(fb.get_ranges()).sum()
    pa, pb = cph.geometry.PointCloud.create_from_laserscanbuffer(fa, 0.5, 10.0), g.PointCloud.create_from_laserscanbuffer(fb, 0.5, 10.0)
    xa, xb = np.asarray(pa.points.cpu(), F), np.asarray(pb.points.cpu(), F)
    assert len(xb) > steps and xa.tobytes() == xb.tobytes()
    assert np.asarray(pa.colors.cpu(), F).tobytes() == np.asarray(pb.colors.cpu(), F).tobytes()
    va = cph.geometry.LaserScanBuffer.create_from_point_cloud(pa, 0.02, 0.0, 1.0, 2, 0.2, 20.0)
    vb = g.LaserScanBuffer.create_from_point_cloud(pb, 0.02, 0.0, 1.0, 2, 0.2, 20.0)
    assert (va.num_steps, va.num_scans, va.num_max_scans) == (vb.num_steps, 2, 50)
    assert np.asarray(va.ranges).tobytes() == vb.get_ranges().tobytes() and (~np.isnan(vb.get_ranges())).sum() > 50
    popped = a.pop_host_one_scan()
    assert np.asarray(popped[0]).tobytes() == b.pop_host_one_scan()[0].tobytes() and a.num_scans == 2
