"""Pass-local checks of the label-model iLQR (include/direct_quad.h) and the scenarios they run over.

After every pass of a stepper (begin / iterate(1) / get), the checker takes the stepper's OWN previous iterate, gains
and flags and recomputes that single pass in np.longdouble with oracle/quad_numpy.py.  Nothing accumulates between
passes, so float storage and rough problems are checkable; an accept / reject decision is asserted only when it is
decidable ("Pass-local checking").  Checks:

  A  one-step roll-out consistency of the stored iterate, in units of eps64 * (|x_k| + dt * sum |terms of f|)
  B  the recorded cost is the cost of the stored iterate (1e-13 relative, both storage types)
  C  gains and regulariser index against backward_with_retry from prev
  D  control law of an accepted pass, knot by knot
  E  the line-search decision, where decidable
  F  invariants that need no decision

Steppers: RefBatch (oracle/quad_ref.c, double), NumpyBatch (the restatement, any storage), DeviceBatch (QuadSolver).
"""
import ctypes as C

import numpy as np

from direct_amd import quad
from oracle import quad_numpy as qn

LD = np.longdouble
EPS64 = LD(2.0) ** -53
SCALARS = qn.SCALARS

# Worst residual of check A over S1..S5 with oracle/quad_ref.c (libm sin / cos, true divisions) as the stepper, in
# the units of check A; tests/test_quad_pass_checks.py asserts that the reference stays within it.  The device is
# allowed 8 x as much: its sincos_fast is 1-2 ulp against libm's < 1, divisions are Newton reciprocals and the
# compiler contracts FMAs.  A wrong term is ~1e10 units.
R_REF = 3.76
A_BOUND_UNITS = 8 * R_REF
COST_RTOL = 1e-13          # tests/test_gpu_quad.py's begin-cost tolerance
GAIN_RTOL = 1e-9           # the project's per-pass gain tolerance, times the largest gain of the trajectory
PIVOT_MIN = 1e-9           # an LLT pivot is decidable at this fraction of its diagonal
KF_NOISE_FLOOR = 1e-5     # max|kf| below this fraction of its terms: 1e-9 of it would be under 1e-14 (90 eps64) of the terms,
                          # which an N-knot sweep in double cannot promise (quad_ref.c itself: up to 4e-16 of the terms)
THETA_MAX = 1.3
# |theta| of the roll-outs that decisions adopt.  S2 is ours to trim and keeps to THETA_MAX.  S1, S4 and S5 are fixed by
# their definition and their reference runs pass it (the label problems tilt to 1.38 on the way, S4 with free inputs to
# 1.53): capped at the values measured with oracle/quad_ref.c, so that no edit moves them closer to the singularity.
THETA_CAP = {"S1": 1.39, "S2": THETA_MAX, "S3": THETA_MAX, "S4": 1.54, "S5": 1.39}
# scenarios whose every decision is decidable with oracle/quad_ref.c as the stepper (tests/test_quad_pass_checks.py
# asserts the list): the device run is also held to whole-run parity with quad_ref.c on these
FULLY_DECIDABLE = ("S1-N40", "S1-N100", "S2-N3", "S2-N7", "S2-N100", "S3-fixed0-f64", "S3-fixed1-f64", "S4")


def params(**kw):
    """default_params of the product library, filled by hand so that CPU tests need no device library"""
    p = quad.Params(0.98, 9.81, (C.c_double * 3)(2.64e-3, 2.64e-3, 4.96e-3), 0.05, 1.0, 0.1, 1.0, 0.05, 0.05, 50.0,
                    1000.0, 500.0, 500.0, 100.0, 4.0, 1e-6, 50, 0)
    for k, v in kw.items():
        if k == "inertia":
            v = (C.c_double * 3)(*v)
        setattr(p, k, v)
    return p


# ------------------------------------------------------------------------------------------------ steppers
class RefBatch:
    """oracle/quad_ref.c, one Stepper per trajectory, stacked"""
    store = np.float64

    def __init__(self, p, N, x0, xg, store=np.float64):
        from oracle import quadapi
        assert np.dtype(store) == np.float64, "quad_ref.c is double-only"
        self.s = [quadapi.Stepper(p, N, x0[b], xg[b]) for b in range(len(x0))]

    def iterate(self, n=1):
        for s in self.s:
            s.iterate(n)

    def get(self):
        g = [s.get() for s in self.s]
        return {k: np.stack([np.asarray(r[k]) for r in g]) for k in g[0]}

    def close(self):
        for s in self.s:
            s.close()


class NumpyBatch:
    def __init__(self, p, N, x0, xg, store=np.float64):
        self.s = qn.Stepper(p, N, np.asarray(x0, store), np.asarray(xg, store), store, np.float64)

    def iterate(self, n=1):
        self.s.iterate(n)

    def get(self):
        return self.s.get()

    def close(self):
        pass


class DeviceBatch:
    def __init__(self, p, N, x0, xg, store=np.float64):
        self.s = quad.QuadSolver(len(x0), N, store)
        self.s.begin(p, x0, xg)

    def iterate(self, n=1):
        self.s.iterate(n)

    def get(self):
        return self.s.get()

    def close(self):
        self.s.close()


# ------------------------------------------------------------------------------------------------ scenarios
class Scenario:
    def __init__(self, name, family, p, N, x0, xg, passes, stores=(np.float64, np.float32), exact=None):
        self.name, self.family, self.p, self.N, self.passes, self.stores, self.exact = name, family, p, N, passes, stores, exact
        self.x0, self.xg = np.ascontiguousarray(x0, np.float64), np.ascontiguousarray(xg, np.float64)

    def inputs(self, store):
        """x0 / xg as the stepper of that storage type receives them (float steppers get float inputs)"""
        return self.x0.astype(store).astype(np.float64), self.xg.astype(store).astype(np.float64)


S2_INERTIA = (2.64e-3, 3.71e-3, 4.96e-3)
# S2: N -> (seed, pool, picks).  N = 7 drops the one start whose adopted roll-outs pass |theta| = 1.3 (1.45).  The long
# horizons are trimmed: of a pool of 40 rough starts, those whose reference run
# keeps the adopted roll-outs clear of the Euler singularity and the backward sweep well conditioned (at most one
# undecidable pass, gains within 1e-10 x scale of the longdouble recomputation); a 5 s horizon from a tumbling
# start otherwise spends most passes near |theta| = pi / 2.
S2_SETS = {1: (2101, 6, range(6)), 2: (2102, 6, range(6)), 3: (2103, 6, range(6)), 7: (2107, 6, (0, 2, 3, 4, 5)),
           40: (2140, 40, (2, 7, 11, 16, 18, 25)), 100: (2200, 40, (2, 4, 6, 18, 21, 23))}
S5_NATURAL_ITERS = 11      # the label problems below exit after at most this many passes (asserted on the CPU)


def s2_problems(batch, seed):
    """general states: yaw anywhere in +-6 rad, tilted, spinning and moving; the goal ~1.5 m away, level and at rest, its
    yaw within +-0.5 of the start's"""
    r = np.random.default_rng(seed)
    x0, xg = np.zeros((batch, 12)), np.zeros((batch, 12))
    x0[:, :3] = r.normal(0, 2.0, (batch, 3))
    x0[:, 3:6] = r.normal(0, 1.0, (batch, 3))
    x0[:, 6:8] = r.uniform(-0.6, 0.6, (batch, 2))
    x0[:, 8] = r.uniform(-6.0, 6.0, batch)
    x0[:, 9:12] = r.normal(0, 0.5, (batch, 3))
    d = r.normal(0, 1, (batch, 3))
    xg[:, :3] = x0[:, :3] + 1.5 * d / np.linalg.norm(d, axis=1, keepdims=True)
    xg[:, 8] = x0[:, 8] + r.uniform(-0.5, 0.5, batch)
    return x0, xg


def scenarios():
    out = []
    for N in (40, 100):                                                            # S1: the existing benign family
        x0, xg = quad.label_problems(4, seed=1000)
        out.append(Scenario("S1-N%d" % N, "S1", params(), N, x0, xg, 50))
    for N, (seed, pool, picks) in S2_SETS.items():                                 # S2: general state, distinct inertia
        x0, xg = (a[list(picks)] for a in s2_problems(pool, seed))
        out.append(Scenario("S2-N%d" % N, "S2", params(inertia=S2_INERTIA), N, x0, xg, 2 if N == 1 else 14))
    hover = np.zeros((2, 12)); hover[:, :3] = ((1.0, -2.0, 1.5), (0.0, 0.0, 0.0))  # S3: stuck at the optimum
    for fixed in (0, 1):
        # mass 1.0: m g (1 / m) is exact.  Float storage also needs the hover input m g to BE a float, or the stored
        # input is not the hover input and the start is no optimum: gravity 9.8125 there.
        out.append(Scenario("S3-fixed%d-f64" % fixed, "S3", params(mass=1.0, iter_max=30, fixed_iters=fixed), 20, hover, hover, 31,
                            stores=(np.float64,), exact="stuck"))
        out.append(Scenario("S3-fixed%d-f32" % fixed, "S3", params(mass=1.0, gravity=9.8125, iter_max=30, fixed_iters=fixed), 20,
                            hover, hover, 31, stores=(np.float32,), exact="stuck"))
    x0, xg = quad.label_problems(4, seed=1000)                                     # S4: singular Quu at the last knot
    out.append(Scenario("S4", "S4", params(r_thrust=0.0, r_torque=0.0, qf_vel=0.0, qf_rate=0.0), 5, x0, xg, 12, exact="singular"))
    x0, xg = quad.label_problems(4, seed=1000)                                     # S5: bench mode, beyond convergence
    out.append(Scenario("S5", "S5", params(iter_max=2 * S5_NATURAL_ITERS, fixed_iters=1), 100, x0, xg, 2 * S5_NATURAL_ITERS,
                        stores=(np.float32,)))
    return out


# ------------------------------------------------------------------------------------------------ the checker
def _half_ulp(v, store):
    if np.dtype(store) == np.float64:
        return LD(0)
    return (np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(LD)) / 2


class PassStats:
    def __init__(self):
        self.passes = self.undecidable = self.c_skipped = 0
        self.steps_decided = set()        # step indices asserted on decidable passes; 11 = all rejected
        self.quadrants, self.negative_k = set(), False
        self.theta_decided = 0.0
        self.a_units = self.c_worst = 0.0
        self.reg_trace, self.step_trace, self.decided_trace = [], [], []

    def merge(self, o):
        self.passes += o.passes; self.undecidable += o.undecidable; self.c_skipped += o.c_skipped
        self.steps_decided |= o.steps_decided; self.quadrants |= o.quadrants
        self.negative_k |= o.negative_k
        self.theta_decided = max(self.theta_decided, o.theta_decided); self.a_units = max(self.a_units, o.a_units); self.c_worst = max(self.c_worst, o.c_worst)


class PassChecker:
    def __init__(self, p, N, xg, store, a_bound_units=A_BOUND_UNITS):
        self.p, self.N, self.store, self.a_bound = p, N, np.dtype(store), a_bound_units
        self.xg = np.asarray(xg, np.float64)
        self.stats = PassStats()

    # -- A and B bind on every stored iterate
    def check_A(self, cur, tag):
        x, u = cur["x"].astype(LD), cur["u"].astype(LD)
        f, fa = qn.dynamics(self.p, x[:, :-1], u, LD, with_abs=True)
        dt = LD(self.p.dt)
        pred = x[:, :-1] + dt * f
        err = np.abs(x[:, 1:] - pred)
        unit = EPS64 * (np.abs(x[:, :-1]) + dt * fa)
        excess = np.maximum(err - _half_ulp(pred, self.store), 0)
        with np.errstate(all="ignore"):
            units = np.where(excess > 0, excess / unit, 0).astype(np.float64)
        worst = float(units.max()) if units.size else 0.0
        self.stats.a_units = max(self.stats.a_units, worst)
        assert worst <= self.a_bound, "%s A: roll-out residual %.3g units > %.3g at (b, k, i) = %s" % (
            tag, worst, self.a_bound, np.unravel_index(units.argmax(), units.shape))
        k = np.rint(cur["x"][:, :, 6:9].astype(np.float64) * (2 / np.pi)).astype(np.int64)
        self.stats.quadrants |= set(np.unique(k & 3).tolist())
        self.stats.negative_k |= bool((k < 0).any())

    def check_B(self, cur, tag):
        c = qn.total_cost(self.p, cur["x"].astype(LD), cur["u"].astype(LD), self.xg, LD)
        bad = ~(np.abs(cur["cost"].astype(LD) - c) <= LD(COST_RTOL) * np.abs(c))
        assert not bad.any(), "%s B: recorded cost %r, cost of the stored iterate %r" % (tag, cur["cost"][bad], c[bad])

    def check_begin(self, cur):
        assert not any(np.isnan(cur[k]).any() for k in ("x", "u", "cost")), "begin: NaN"
        self.check_A(cur, "begin")
        self.check_B(cur, "begin")
        assert not cur["iter"].any() and not cur["done"].any() and not cur["reg"].any() and not cur["fwd_passes"].any()

    def check_pass(self, prev, cur, it=0):
        p, tag = self.p, "pass %d" % it
        B = len(cur["cost"])
        for k in ("x", "u", "K", "kf") + SCALARS:
            assert not np.isnan(cur[k]).any(), "%s F: NaN in %s" % (tag, k)
        idle = (prev["done"] != 0) | (prev["iter"] >= p.iter_max)
        act = np.flatnonzero(~idle)
        for b in np.flatnonzero(idle):                                             # F: a finished trajectory does not move
            for k in ("x", "u", "cost", "reg", "step", "fp_failed", "iter", "fwd_passes"):
                assert np.array_equal(cur[k][b], prev[k][b]), "%s F: finished trajectory %d changed its %s" % (tag, b, k)
            assert cur["done"][b] == 1
        self.check_A(cur, tag)
        self.check_B(cur, tag)
        if act.size == 0:
            return
        pv = {k: prev[k][act] for k in prev}
        cu = {k: cur[k][act] for k in cur}
        xg = self.xg[act]
        acc = cu["fp_failed"] == 0
        # ---- F
        assert np.array_equal(cu["iter"], pv["iter"] + 1) and np.array_equal(cu["fwd_passes"], pv["fwd_passes"] + 1), tag + " F: counters"
        assert set(np.unique(cu["fp_failed"])) <= {0.0, 1.0} and set(np.unique(cu["bp_failed"])) <= {0.0, 1.0}
        assert (cu["cost"][acc] < pv["cost"][acc]).all(), tag + " F: accepted without a strict decrease"
        for b in np.flatnonzero(~acc):
            assert (np.array_equal(cu["x"][b], pv["x"][b]) and np.array_equal(cu["u"][b], pv["u"][b])
                    and cu["cost"][b] == pv["cost"][b]), "%s F: rejected pass moved trajectory %d" % (tag, act[b])
        conv = (not p.fixed_iters) & acc & (pv["cost"] - cu["cost"] <= p.tol * pv["cost"])
        exp_done = conv | (cu["iter"] >= p.iter_max)
        assert np.array_equal(cu["done"] != 0, exp_done), "%s F: done %s, expected %s" % (tag, cu["done"], exp_done)
        assert ((cu["step"] >= 0) & (cu["step"] <= 10) & (cu["reg"] >= 0) & (cu["reg"] <= qn.REG_MAX)).all(), tag + " F: step / reg range"
        # ---- C
        aux = {}
        K, kf, reg, bp, piv, retries = qn.backward_with_retry(p, pv["x"], pv["u"], xg, pv["reg"], pv["step"], pv["fp_failed"],
                                                              pv["bp_failed"], self.store, LD, aux)
        plain = (pv["fp_failed"] != 0) & (retries == 0) & (cu["bp_failed"] == 0)
        want = np.minimum(pv["reg"] + 1, qn.REG_MAX)
        assert np.array_equal(cu["reg"][plain], want[plain]), "%s C: reg %s after a failed line search from %s" % (
            tag, cu["reg"][plain], pv["reg"][plain])
        sure = piv >= PIVOT_MIN
        assert np.array_equal(cu["reg"][sure], reg[sure]), "%s C: reg %s, recomputed %s (retries %s)" % (tag, cu["reg"], reg, retries)
        assert np.array_equal(cu["bp_failed"][sure], bp[sure]), tag + " C: bp_failed"
        for b in range(act.size):
            if cu["reg"][b] != reg[b] or bp[b]:
                self.stats.c_skipped += 1                                          # undecidable pivot took the other branch
                continue
            # scale: the largest gain of the trajectory, as in tests/test_gpu_quad.py.  At an optimum kf cancels to rounding
            # noise and its own size is no scale for its error: below KF_NOISE_FLOOR x the size of the terms it is the sum of
            # (quad_numpy.backward's kf_scale) that floor is the scale, i.e. never less than 1e-14 x the terms.
            kf_ref_scale = max(np.abs(kf[b]).max(), LD(KF_NOISE_FLOOR) * aux["kf_scale"][b])
            for name, got, ref, scale in (("K", cu["K"][b], K[b], np.abs(K[b]).max()), ("kf", cu["kf"][b], kf[b], kf_ref_scale)):
                d = np.maximum(np.abs(got.astype(LD) - ref) - _half_ulp(ref, self.store), 0)
                worst = float(d.max() / scale) if scale > 0 else (0.0 if d.max() == 0 else np.inf)
                self.stats.c_worst = max(self.stats.c_worst, worst)
                assert worst <= GAIN_RTOL, "%s C: %s of trajectory %d off by %.3g x its scale at %s" % (
                    tag, name, act[b], worst, np.unravel_index(d.argmax(), d.shape))
        # ---- D
        cK, ckf = cu["K"].astype(LD), cu["kf"].astype(LD)
        dx = cu["x"].astype(LD)[:, :-1] - pv["x"].astype(LD)[:, :-1]
        alpha = (LD(0.5) ** cu["step"].astype(LD))[:, None, None]
        fb_terms = cK * dx[:, :, None, :]
        upred = pv["u"].astype(LD) + alpha * ckf + fb_terms.sum(-1)
        tol = _half_ulp(upred, self.store) + LD(self.a_bound) * EPS64 * (np.abs(pv["u"].astype(LD)) + np.abs(alpha * ckf) + np.abs(fb_terms).sum(-1))
        d = np.abs(cu["u"].astype(LD) - upred)
        badD = (d > tol) & acc[:, None, None]
        assert not badD.any(), "%s D: u is not prev.u + 2^-step kf + K dx at (b, k, i) = %s (off by %.3g)" % (
            tag, np.argwhere(badD)[0], float(d[badD].max()))
        # ---- E
        Xl, _, cl = qn.trial_costs(p, pv["x"], pv["u"], cu["K"], cu["kf"], xg, self.store, LD)
        _, _, cd = qn.trial_costs(p, pv["x"], pv["u"], cu["K"], cu["kf"], xg, self.store, np.float64)
        old = pv["cost"].astype(LD)
        with np.errstate(all="ignore"):
            dist = np.abs(cl - old)
            fin = np.isfinite(cl) & np.isfinite(cd)
            dec = np.where(fin, (np.abs(cl - cd.astype(LD)) <= dist / 16) & (dist >= LD(1e-12) * old), ~np.isfinite(cl) & ~np.isfinite(cd))
            ok = cl < old
            theta = np.abs(Xl[..., 7]).max(-1).astype(np.float64)                  # [11, B]
        decided = np.ones(B, bool)
        for b in range(act.size):
            first = int(ok[:, b].argmax()) if ok[:, b].any() else 11
            upto = min(first, 10) + 1
            self.stats.passes += 1
            if not dec[:upto, b].all():
                self.stats.undecidable += 1
                decided[act[b]] = False
                continue
            if first < 11:                                                         # the roll-out this decision adopts
                self.stats.theta_decided = max(self.stats.theta_decided, float(theta[first, b]))
            self.stats.steps_decided.add(first)
            if first == 11:
                assert cu["fp_failed"][b] == 1, "%s E: trajectory %d accepted step %d, every trial costs more (decidable)" % (
                    tag, act[b], cu["step"][b])
            else:
                assert cu["fp_failed"][b] == 0 and cu["step"][b] == first, "%s E: trajectory %d took step %s (fp_failed %d), decidably %d" % (
                    tag, act[b], cu["step"][b], cu["fp_failed"][b], first)
        self.stats.decided_trace.append(decided)
        self.stats.reg_trace.append(cur["reg"].copy())
        self.stats.step_trace.append(np.where(cur["fp_failed"] != 0, 11, cur["step"]))


def _get(stepper):
    g = stepper.get()
    out = {}
    for k, nd in (("x", 3), ("u", 3), ("K", 4), ("kf", 3)):
        a = np.asarray(g[k])
        out[k] = a[None] if a.ndim == nd - 1 else a
    for k in SCALARS:
        out[k] = np.atleast_1d(np.asarray(g[k], np.float64))
    return out


def run_checked(stepper, scen, store, a_bound_units=A_BOUND_UNITS, wrap=None, log=None):
    """begin has happened in the stepper's constructor; runs scen.passes passes (or until all are done) under the checker.
    `wrap(state, pass_index)` may alter what get() returned (planted faults).  Returns the stats and the last state."""
    _, xg = scen.inputs(store)
    ck = PassChecker(scen.p, scen.N, xg, store, a_bound_units)
    grab = (lambda i: wrap(_get(stepper), i)) if wrap else (lambda i: _get(stepper))
    cur = grab(0)
    assert np.dtype(cur["x"].dtype) == np.dtype(store)
    ck.check_begin(cur)
    first = cur
    for it in range(1, scen.passes + 1):
        prev = cur
        stepper.iterate(1)
        cur = grab(it)
        ck.check_pass(prev, cur, it)
        if log:
            log("%s %s pass %d: step %s reg %s cost %s A %.2f" % (scen.name, np.dtype(store).name, it, ck.stats.step_trace[-1] if ck.stats.step_trace else "-",
                                                                 cur["reg"], cur["cost"], ck.stats.a_units))
        if (cur["done"] != 0).all():
            break
    if scen.exact == "stuck":
        check_stuck(scen, first, cur, ck.stats)
    if scen.exact == "singular":
        assert (ck.stats.reg_trace[0] == 1).all(), "S4: the zero Quu of the last knot must fail at reg 0 and be retried at reg 1"
        assert len(ck.stats.steps_decided & {4, 5, 6, 7}) >= 3, "S4 must decide steps above 3 (step > 3 -> reg + 1)"
    return ck.stats, cur


def check_stuck(scen, first, last, stats):
    """S3 exactly: cost 0, the begin roll untouched, every line search fails, reg climbs 0, 1, .., 24 and holds, exit by
    iter_max with iters == 30"""
    assert (first["cost"] == 0.0).all() and (last["cost"] == 0.0).all()
    assert np.array_equal(first["x"], last["x"]) and np.array_equal(first["x"], np.broadcast_to(first["x"][:, :1], first["x"].shape))
    assert (last["iter"] == 30).all() and (last["fwd_passes"] == 30).all() and (last["done"] == 1).all()
    regs, steps = np.array(stats.reg_trace[:30]), np.array(stats.step_trace[:30])
    assert (steps == 11).all(), steps
    assert np.array_equal(regs, np.broadcast_to(np.minimum(np.arange(30), 24)[:, None], regs.shape)), regs


def assert_conditions(by_family, total):
    """what the scenario set must meet, so that a later edit cannot hollow the tests out"""
    for fam in ("S1", "S2", "S4"):
        st = by_family[fam]
        assert st.passes > 0 and st.undecidable <= 0.10 * st.passes, "%s: %d of %d passes undecidable" % (fam, st.undecidable, st.passes)
    for fam, st in by_family.items():
        assert st.theta_decided <= THETA_CAP[fam], "%s: a decision adopts a roll-out with |theta| = %.3f" % (fam, st.theta_decided)
    assert total.c_skipped == 0
    assert set(range(6)) | {11} <= total.steps_decided, "step indices decided: %s" % sorted(total.steps_decided)
    assert total.quadrants == {0, 1, 2, 3} and total.negative_k, (total.quadrants, total.negative_k)
