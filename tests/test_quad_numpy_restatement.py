"""The NumPy restatement of the label model (oracle/quad_numpy.py) in float64 against oracle/quad_ref.c, function by
function and pass by pass, and against things that depend on neither: a longdouble finite difference of its
Jacobians and the exact trace of the stuck scenario."""
import numpy as np

from tests import quad_pass_lib as L
from oracle import quad_numpy as qn
from oracle import quadapi


def _general_states(n, seed):
    r = np.random.default_rng(seed)
    x = np.concatenate([r.normal(0, 2, (n, 3)), r.normal(0, 1, (n, 3)), r.uniform(-0.9, 0.9, (n, 2)), r.uniform(-6, 6, (n, 1)),
                        r.normal(0, 1, (n, 3))], axis=1)
    u = np.array([9.0, 0, 0, 0]) + r.normal(0, 1, (n, 4)) * (2.0, 0.05, 0.05, 0.05)
    return x, u


def test_dynamics_and_jacobians_match_the_reference():
    p = L.params(inertia=L.S2_INERTIA)
    x, u = _general_states(40, 7)
    A, B = qn.jacobians(p, x, u)
    xn = qn.step(p, x, u)
    for i in range(len(x)):
        rA, rB = quadapi.jacobians(p, x[i], u[i])
        # both are double evaluations of the same smooth functions: a few ulps of their largest terms
        assert np.abs(xn[i] - quadapi.step(p, x[i], u[i])).max() < 1e-13 * (1 + np.abs(xn[i]).max())
        assert np.abs(A[i] - rA).max() < 1e-13 * np.abs(rA).max() and np.abs(B[i] - rB).max() < 1e-13 * np.abs(rB).max()
    assert np.abs(x[:, 8]).max() > 3 and np.abs(x[:, 9:]).max() > 1


def test_jacobians_match_a_longdouble_finite_difference():
    p = L.params(inertia=L.S2_INERTIA)
    x, u = _general_states(10, 8)
    A, B = qn.jacobians(p, x, u)
    Al, Bl = qn.jacobians(p, x, u, np.longdouble)
    h = np.longdouble(1e-5)
    xl, ul = x.astype(np.longdouble), u.astype(np.longdouble)
    for j in range(12):
        e = np.zeros(12, np.longdouble); e[j] = h
        fd = (qn.step(p, xl + e, ul, np.longdouble) - qn.step(p, xl - e, ul, np.longdouble)) / (2 * h)
        assert np.abs(fd - A[:, :, j]).max() < 1e-8 and np.abs(fd - Al[:, :, j]).max() < 1e-8
    for j in range(4):
        e = np.zeros(4, np.longdouble); e[j] = h
        fd = (qn.step(p, xl, ul + e, np.longdouble) - qn.step(p, xl, ul - e, np.longdouble)) / (2 * h)
        assert np.abs(fd - B[:, :, j]).max() < 1e-8
    assert np.abs(A - Al.astype(np.float64)).max() < 1e-13 * np.abs(A).max()


def test_next_reg_is_the_schedule():
    assert qn.next_reg(0, 0, 0, 0) == 0 and qn.next_reg(3, 0, 0, 0) == 2 and qn.next_reg(3, 2, 0, 0) == 3
    assert qn.next_reg(3, 3, 0, 0) == 3 and qn.next_reg(3, 4, 0, 0) == 4 and qn.next_reg(3, 0, 1, 0) == 4
    assert qn.next_reg(3, 0, 0, 1) == 4 and qn.next_reg(24, 7, 1, 1) == 24
    assert np.array_equal(qn.next_reg([0, 24], [0, 10], [0, 0], [0, 0]), [0, 24])


def test_stepwise_against_the_reference_while_decidable():
    """S1 to S4 pass by pass.  A trajectory is compared until its first pass that the checker (run on the reference)
    finds undecidable: from there the two may part ways.  Decisions and flags are compared on every such pass, and the
    cost to 1e-8.  Gains, cost and iterate are held to the per-pass tolerances of tests/test_gpu_quad.py over the four
    passes that test runs on S1, and over the first pass on S2 to S4: two parallel runs of a rough problem drift apart
    with every pass (S2-N100 is 3e-10 of the cost apart after its second pass, against the 1e-10 there), which is what
    the pass-local checker is for; it holds every pass of the reference to the longdouble recomputation."""
    compared = 0
    DRIFT = 1e-8
    for sc in L.scenarios():
        if np.float64 not in sc.stores or sc.family == "S5":
            continue
        x0, xg = sc.inputs(np.float64)
        ref, mine = L.RefBatch(sc.p, sc.N, x0, xg), qn.Stepper(sc.p, sc.N, x0, xg)
        ck = L.PassChecker(sc.p, sc.N, xg, np.float64)
        r, g = L._get(ref), mine.get()
        assert np.abs(g["cost"] - r["cost"]).max() <= 1e-13 * np.abs(r["cost"]).max() and np.abs(g["x"] - r["x"]).max() < 1e-12
        alive = np.ones(len(x0), bool)
        for it in range(1, sc.passes + 1):
            prev = r
            ref.iterate(1); mine.iterate(1)
            r, g = L._get(ref), mine.get()
            ck.check_pass(prev, r, it)
            if ck.stats.decided_trace and len(ck.stats.decided_trace) == it:
                alive &= ck.stats.decided_trace[-1]
            for b in np.flatnonzero(alive & (prev["done"] == 0)):
                for k in ("step", "reg", "fp_failed", "bp_failed", "iter", "done"):
                    assert g[k][b] == r[k][b], (sc.name, it, b, k, g[k][b], r[k][b])
                compared += 1
                assert abs(g["cost"][b] - r["cost"][b]) <= DRIFT * abs(r["cost"][b])
                if it > (4 if sc.family == "S1" else 1):
                    continue
                sK, sk = np.abs(r["K"][b]).max(), np.abs(r["kf"][b]).max()
                assert np.abs(g["K"][b] - r["K"][b]).max() <= 1e-9 * sK, (sc.name, it, b)
                if sk > 1e-6:                                                      # at the optimum kf is rounding noise
                    assert np.abs(g["kf"][b] - r["kf"][b]).max() <= 1e-9 * sk, (sc.name, it, b)
                assert abs(g["cost"][b] - r["cost"][b]) <= 1e-10 * abs(r["cost"][b])
                for k in ("x", "u"):                                               # 1e-9 as there, times the size where it exceeds 1
                    assert np.abs(g[k][b] - r[k][b]).max() < 1e-9 * max(1.0, np.abs(r[k][b]).max()), (sc.name, it, b, k)
            if (r["done"] != 0).all():
                break
        ref.close()
    assert compared > 300


def test_stuck_scenario_trace_is_exact_in_both_storage_types():
    for sc in L.scenarios():
        if sc.family == "S3":
            for store in sc.stores:
                st, cur = L.run_checked(L.NumpyBatch(sc.p, sc.N, *sc.inputs(store), store), sc, store)   # check_stuck inside
                assert st.steps_decided == {11}


def test_solve_is_the_stepper_run_to_the_end():
    sc = [s for s in L.scenarios() if s.name == "S2-N7"][0]
    x0, xg = sc.inputs(np.float64)
    out = qn.solve(sc.p, x0, xg, sc.N)
    r = quadapi.solve_batch(sc.p, sc.N, x0, xg)
    assert out["x"].shape == r["x"].shape and (out["iters"] <= sc.p.iter_max).all()
    assert (out["cost"] < qn.get(qn.begin(sc.p, x0, xg, sc.N, np.float64))["cost"]).all()
