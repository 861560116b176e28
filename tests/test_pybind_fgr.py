"""FeatureFPFH / FeatureSHOT, FastGlobalRegistrationOption and the two functions of the reference's pybind11 module
(cupoch_amd/cpp/src/pybind_module.cpp) and of the ctypes mirror: names, defaults, both Feature classes and a round trip
of `data` (on the GPU: it lives in device memory).  Skips only where there is nothing to build the module with."""
import copy

import numpy as np
import pytest

DEFAULTS = dict(division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
                iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000)


def module():
    import importlib.util
    import shutil
    missing = [n for n in ("make", "g++") if shutil.which(n) is None] + ([] if importlib.util.find_spec("pybind11") else ["pybind11"])
    if missing:                 # nothing to build the module with: the only reason to skip
        pytest.skip("cupoch_pybind cannot be built here: no %s" % ", ".join(missing))
    from cupoch_amd import pybind as cph        # (a build or an import that breaks is a failure)
    return cph


def test_names_and_defaults_on_both_surfaces():
    cph = module()
    from cupoch_amd import registration as mirror
    for r in (cph.registration, mirror):
        o = r.FastGlobalRegistrationOption()
        for k, v in DEFAULTS.items():
            assert getattr(o, k) == (pytest.approx(v) if isinstance(v, float) else v), k
        o = r.FastGlobalRegistrationOption(division_factor=2.0, use_absolute_scale=True, decrease_mu=False,
                                           maximum_correspondence_distance=0.5, iteration_number=3, tuple_scale=0.9, maximum_tuple_count=7)
        assert (o.use_absolute_scale, o.decrease_mu, o.iteration_number, o.maximum_tuple_count) == (True, False, 3, 7)
        o.iteration_number = 5                                                               # read-write
        c = copy.copy(o)
        c.iteration_number = 6
        assert (o.iteration_number, c.iteration_number) == (5, 6)
        assert "registration::FastGlobalRegistrationOption class" in repr(o) and "iteration_number=5" in repr(o)
        for name, dim in (("FeatureFPFH", 33), ("FeatureSHOT", 352)):
            f = getattr(r, name)()
            assert f.dimension() == dim and f.num() == 0
            assert "registration::Feature class with dimension = %d and num = 0" % dim in repr(f)
        assert callable(r.registration_fast_based_on_feature_matching) and callable(r.correspondences_from_features)
    doc = cph.registration.registration_fast_based_on_feature_matching.__doc__
    assert doc.count("source_feature") == 2 and "FeatureFPFH" in doc and "FeatureSHOT" in doc       # both overloads


@pytest.mark.gpu
def test_feature_data_round_trip():
    cph = module()
    rng = np.random.default_rng(2)
    for name, dim in (("FeatureFPFH", 33), ("FeatureSHOT", 352)):
        F = getattr(cph.registration, name)
        f = F()
        f.resize(4)
        assert f.num() == 4 and np.asarray(f.data).shape == (4, dim)
        a = rng.standard_normal((9, dim)).astype(np.float32)
        f.data = a
        assert f.num() == 9 and np.asarray(f.data).tobytes() == a.tobytes()
        g = copy.deepcopy(f)
        f.resize(2)
        assert g.num() == 9 and np.asarray(g.data).tobytes() == a.tobytes() and f.num() == 2
        with pytest.raises(ValueError):
            f.data = np.zeros((3, dim + 1), np.float32)
