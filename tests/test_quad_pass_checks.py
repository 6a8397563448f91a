"""The pass checker of tests/quad_pass_lib.py on the CPU: it runs clean over every scenario with oracle/quad_ref.c
as the stepper (and with the NumPy restatement for float storage, which quad_ref.c does not have), the scenario set
meets its conditions with the reference alone, and every planted fault is caught.  The planted faults are thin
wrappers around get(): they prove that tests/test_gpu_quad_passes.py would notice a subtly wrong kernel."""
import numpy as np
import pytest

from tests import quad_pass_lib as L
from oracle import quad_numpy as qn

# scenarios whose every decision is decidable with quad_ref.c: tests/test_gpu_quad_passes.py also asserts whole-run
# parity with quad_ref.c on these
FULLY_DECIDABLE = L.FULLY_DECIDABLE


def _run(sc, store, cls, **kw):
    st = cls(sc.p, sc.N, *sc.inputs(store), store)
    try:
        return L.run_checked(st, sc, store, **kw)
    finally:
        st.close()


def test_checker_runs_clean_and_the_scenario_set_meets_its_conditions():
    fam, total, full, r_ref = {}, L.PassStats(), [], 0.0
    for sc in L.scenarios():
        stores = sc.stores + (np.float64,) if sc.family == "S5" else sc.stores         # r_ref is measured over S5 too
        for store in stores:
            ref = np.dtype(store) == np.float64
            st, cur = _run(sc, store, L.RefBatch if ref else L.NumpyBatch)
            print("%-14s %-7s passes %3d undecidable %2d adopted |theta| %.3f A %.2f units, gains %.1e x scale, steps %s" % (
                sc.name, np.dtype(store).name, st.passes, st.undecidable, st.theta_decided, st.a_units, st.c_worst, sorted(st.steps_decided)))
            if not ref:
                continue                                                             # the conditions are the reference's alone
            r_ref = max(r_ref, st.a_units)
            fam.setdefault(sc.family, L.PassStats()).merge(st)
            total.merge(st)
            if st.undecidable == 0 and store in sc.stores:
                full.append(sc.name)
            if sc.name == "S4":                                                      # the trace of the first trajectory, pinned
                assert [int(t[0]) for t in st.step_trace[:8]] == [6, 7, 5, 2, 2, 3, 4, 2]
                assert [int(t[0]) for t in st.reg_trace[:8]] == [1, 2, 3, 4, 4, 4, 4, 5]
            if sc.name == "S1-N100":
                assert cur["iter"].max() == L.S5_NATURAL_ITERS                       # S5 runs twice this many passes
    print("r_ref = %.3f units" % r_ref)
    assert r_ref <= L.R_REF
    L.assert_conditions(fam, total)
    assert sorted(full) == sorted(FULLY_DECIDABLE), full


# ---------------------------------------------------------------------------------------------- planted faults
def _scen(name):
    return [s for s in L.scenarios() if s.name == name][0]


def _scale_one_K(g, it):
    if it >= 1:
        i = np.unravel_index(np.abs(g["K"][0]).argmax(), g["K"][0].shape)
        g["K"][0][i] *= 1 + 1e-6
    return g


def _negate_kf(g, it):
    if it >= 1:
        g["kf"][1, g["kf"].shape[1] // 2] *= -1
    return g


def _shift_cost(g, it):
    g["cost"] = g["cost"] * (1 + 1e-9)
    return g


def _step_one_high(g, it):
    if it >= 1:
        g["step"] = np.where(g["fp_failed"] == 0, g["step"] + 1, g["step"])
    return g


def _reg_unclamped(g, it):
    if it >= 1:
        g["reg"] = np.full_like(g["reg"], it - 1)        # what S3's reg is without the clamp to 24
    return g


def _move_x(g, it):
    if it == 2:
        x = g["x"]
        x[2, 3, 4] = np.nextafter(np.nextafter(np.nextafter(np.nextafter(x[2, 3, 4], np.inf, dtype=x.dtype), np.inf, dtype=x.dtype),
                                               np.inf, dtype=x.dtype), np.inf, dtype=x.dtype)
    return g


def _drop_gyro_term(sc):
    """x re-rolled from u with the (J1 - J0) w0 w1 term of omegadot_z dropped"""
    def wrap(g, it):
        x = g["x"].astype(np.float64)
        J = sc.p.inertia
        for k in range(sc.N):
            f = qn.dynamics(sc.p, x[:, k], g["u"][:, k].astype(np.float64))
            f[:, 11] += (J[1] - J[0]) * x[:, k, 9] * x[:, k, 10] / J[2]
            x[:, k + 1] = x[:, k] + sc.p.dt * f
        g["x"] = x.astype(g["x"].dtype)
        return g
    return wrap


FAULTS = [("K entry scaled by 1 + 1e-6", "S2-N7", np.float64, _scale_one_K, r" C: K "),
          ("kf negated at one knot", "S2-N7", np.float64, _negate_kf, r" C: kf "),
          ("cost shifted by 1e-9", "S2-N7", np.float64, _shift_cost, r" B: "),
          ("cost shifted by 1e-9, float storage", "S2-N7", np.float32, _shift_cost, r" B: "),
          ("step reported one too high", "S2-N7", np.float64, _step_one_high, r" [DE]: "),
          ("reg not clamped", "S3-fixed1-f64", np.float64, _reg_unclamped, r"reg"),
          # four double ulps of an entry are within check A's bound in its own units (8 of 30); the storage ulp that
          # matters is the float one, where the derived half-ulp allowance leaves no room for four
          ("x entry moved by 4 storage ulps", "S2-N7", np.float32, _move_x, r" A: "),
          ("J1 - J0 term dropped", "S2-N7", np.float64, None, r" A: ")]


@pytest.mark.parametrize("what,scen,store,wrap,where", FAULTS, ids=[f[0].replace(" ", "_") for f in FAULTS])
def test_planted_fault_is_caught(what, scen, store, wrap, where):
    sc = _scen(scen)
    ref = np.dtype(store) == np.float64
    _run(sc, store, L.RefBatch if ref else L.NumpyBatch)                            # clean without the fault
    with pytest.raises(AssertionError, match=where):
        _run(sc, store, L.RefBatch if ref else L.NumpyBatch, wrap=wrap or _drop_gyro_term(sc))
