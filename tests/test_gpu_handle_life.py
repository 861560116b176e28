"""The life of the five handle kinds of the C ABI (TSDF volume, scalable TSDF volume, occupancy grid, distance transform,
stereo matcher), each at its smallest legal size: a handle belongs to the context that made it, is destroyed once, a null
handle is nothing to destroy, and a context takes its live handles with it."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

# kind -> (make(engine) -> handle, the destroy entry point, its refusal, a call of the owner's that must still succeed)
KINDS = {
    "tsdf": (lambda e: e.tsdf_create(1.0, 3, 0.1, 0), "mi_icp_tsdf_destroy", "tsdf_destroy: not a volume of this context",
             lambda e, h: e.tsdf_reset(h)),
    "stsdf": (lambda e: e.stsdf_create(0.01, 0.04, 0, 1, 1), "mi_icp_stsdf_destroy", "stsdf_destroy: not a volume of this context",
              lambda e, h: e.stsdf_num_units(h)),
    "occgrid": (lambda e: e.occgrid_create(2), "mi_icp_occgrid_destroy", "occgrid_destroy: not a grid of this context",
                lambda e, h: e.occgrid_reset(h)),
    "dt": (lambda e: e.dt_create(2), "mi_icp_dt_destroy", "dt_destroy: not a distance transform of this context",
           lambda e, h: e.dt_reconstruct(h, 2)),
    "sgm": (lambda e: e.sgm_create(8, 8, disp_size=64), "mi_icp_sgm_destroy", "sgm_destroy: not a matcher of this context",
            lambda e, h: sgm_is_known(e, h)),
}


def sgm_is_known(e, h):
    """a matcher without a frame is turned away for that, behind the handle check"""
    from cupoch_amd import MiIcpError
    with pytest.raises(MiIcpError, match="sgm_get_sums: no frame has been processed"):
        e.sgm_get_sums(h, 8, 8, 64)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_handle_belongs_to_its_context_and_is_destroyed_once(kind):
    from cupoch_amd.engine import Engine
    make, destroy_name, refusal, use = KINDS[kind]
    owner, other = Engine(0), Engine(0)
    try:
        L = owner._L
        destroy = getattr(L, destroy_name)
        h = make(owner)
        assert destroy(other._ctx, h) == -1
        assert L.mi_icp_last_error(other._ctx).decode() == refusal
        use(owner, h)                                            # still the owner's, and whole
        assert destroy(owner._ctx, None) == 0 and destroy(other._ctx, None) == 0
        assert destroy(owner._ctx, h) == 0
        assert destroy(owner._ctx, h) == -1
        assert L.mi_icp_last_error(owner._ctx).decode() == refusal
    finally:
        owner.close()
        other.close()


def test_a_context_takes_one_live_handle_of_each_kind_with_it():
    from cupoch_amd.engine import Engine
    eng = Engine(0)
    handles = [KINDS[k][0](eng) for k in sorted(KINDS)]
    assert all(h.value for h in handles)
    eng.close()
    again = Engine(0)                                            # the device is in order after it
    again.synchronize()
    again.close()
