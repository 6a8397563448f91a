"""The label-model kernels (direct_amd/csrc/direct_quad.hip) pass by pass from the device's own state: after every
iterate(1) the checker of tests/quad_pass_lib.py recomputes that single pass in np.longdouble from the device's
previous iterate, gains and flags (checks A to F there), over S1 to S5 in both storage types.  Where the CPU run found
every decision of a scenario decidable (quad_pass_lib.FULLY_DECIDABLE, asserted in tests/test_quad_pass_checks.py) the
device run is also held to whole-run parity with oracle/quad_ref.c at the tolerances of tests/test_gpu_quad.py.

Check A's bound in float64, in units of eps64 * (|x_k| + dt * sum |terms of f|):
  r_ref  = 3.757  worst residual of oracle/quad_ref.c (libm sin / cos, true divisions) over S1 to S5, recorded as 3.76
  bound  = 30.08  8 x r_ref (sincos_fast at 1-2 ulp, Newton reciprocals, contracted FMAs)
  device = printed by every test below next to the bound it is asserted against
Everything else is derived (storage half-ulps) or the project's (1e-13 cost, 1e-9 x scale gains).
"""
import numpy as np
import pytest

from tests import quad_pass_lib as L

pytestmark = pytest.mark.gpu

CASES = [(sc, store) for sc in L.scenarios() for store in sc.stores]


@pytest.mark.parametrize("sc,store", CASES, ids=["%s-%s" % (sc.name, np.dtype(st).name) for sc, st in CASES])
def test_every_pass_from_the_devices_own_state(built, sc, store):
    x0, xg = sc.inputs(store)
    assert len(x0) <= 64                                  # direct_quad_get copies per trajectory
    dev = L.DeviceBatch(sc.p, sc.N, x0, xg, store)
    try:
        st, cur = L.run_checked(dev, sc, store, log=print)
    finally:
        dev.close()
    print("%s %s: passes %d, undecidable %d, adopted |theta| %.3f, A worst %.3f units (bound %.2f), gains worst %.2e x scale, steps decided %s" % (
        sc.name, np.dtype(store).name, st.passes, st.undecidable, st.theta_decided, st.a_units, L.A_BOUND_UNITS, st.c_worst,
        sorted(st.steps_decided)))
    assert st.passes > 0 and st.c_skipped == 0
    if sc.name in L.FULLY_DECIDABLE and np.dtype(store) == np.float64:
        ref = L.RefBatch(sc.p, sc.N, x0, xg)
        ref.iterate(int(cur["iter"].max()))
        r = L._get(ref)
        ref.close()
        assert np.array_equal(cur["iter"], r["iter"]) and np.array_equal(cur["fwd_passes"], r["fwd_passes"])
        assert np.array_equal(cur["step"], r["step"]) and np.array_equal(cur["reg"], r["reg"])
        assert (np.abs(cur["cost"] - r["cost"]) <= 1e-9 * np.abs(r["cost"])).all()
        assert np.abs(cur["x"] - r["x"]).max() < 1e-7 and np.abs(cur["u"] - r["u"]).max() < 1e-6
