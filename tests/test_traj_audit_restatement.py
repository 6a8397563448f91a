"""The arithmetic of direct_traj_audit_batch (direct_amd/csrc/traj_audit_math.h, compiled here by g++: tests/traj_audit_harness.py)
against the exact fixture tests/golden/audit_cases.npz (rationals + mpmath at 60 digits, tests/golden/make_audit_golden.py).

Tolerance, derived, not tuned: |peak - exact| <= 24 u F, u = 2^-53, F the item's absolute companion at the end of
its interval (tests/traj_audit_lib.py, tolerances).  Worst observed on the fixture, in units of u F (every test prints its own): 2.1 on the
synthetic rows, 1.3 on solved plans from poly, 0.005 from bez (whose F is large)."""
import os

import numpy as np
import pytest

from tests import helpers
from tests import traj_audit_harness as H
from tests import traj_audit_lib as L

FIX = np.load(os.path.join(helpers.GOLDEN_DIR, "audit_cases.npz"))
CASES = [str(c) for c in FIX["cases"]]
PLAN_CASES = [str(c) for c in FIX["plan_cases"]]


def case(name):
    return L.fixture_case(FIX, name, helpers.GOLDEN_DIR)


def inputs(c):
    return dict(n_seg=c["n_seg"], T=c["T"], coef=c["coef"], src=c["src"], n_planes=c["n_planes"], planes=c["planes"])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("audit_math"))


def exact_err(got, c, f):
    """|got - (hi + lo)|: got - hi is exact for neighbours (Sterbenz), lo is below an ulp of hi"""
    return np.abs((got - c[f]) - c[f + "_lo"])


@pytest.mark.parametrize("name", CASES)
def test_compiled_math_against_the_exact_fixture(harness, name, record_property):
    c = case(name)
    r = H.run(harness, **inputs(c))
    tol = L.tolerances(c["n_seg"], c["T"], c["coef"], c["src"], c["n_planes"], c["planes"])
    assert np.array_equal(r["status"], c["status"])
    want = np.where(c["status"] == 0, 0, L.INVALID)
    clear = np.ones(len(want), bool)
    if c["planes"] is not None:     # clearance 0: the curve may touch a plane; a touch within the tolerance may go either way
        want = np.where((c["status"] == 0) & (c["cpeak"] > 0), L.CORRIDOR, want)
        clear = np.abs(c["cpeak"]) > tol["cpeak"]
    assert np.array_equal(r["verdict"][clear], want[clear])
    assert np.array_equal(r["t_total"], c["t_total"])
    ok = c["status"] == 0
    assert ok.any()
    fields = [f for f in L.ROW_FIELDS if f in c] + ["gap", "seg_peak"]
    worst = 0.0
    for f in fields:
        err = exact_err(r[f], c, f)
        units = (err / np.maximum(tol[f], 1e-320) * L.TOL_UNITS)[ok]
        print(name, f, "worst error in units of u F: %.3g" % units.max())
        worst = max(worst, float(units.max()))
        assert (err[ok] <= tol[f][ok]).all(), (f, units.max())
        assert (r[f][~ok] == 0).all(), f            # invalid rows: zeros
    record_property("worst_units", worst)
    if c["planes"] is not None:
        assert np.array_equal(r["c_where"], c["c_where"])
        assert (r["at"][~ok] == 0).all()
    else:
        assert (r["cpeak"] == 0).all() and (r["c_where"] == 0).all() and (r["at"][:, 3] == 0).all()
    assert (r["slowdown"][ok] == 1.0).all() and (r["slowdown"][~ok] == 0.0).all()   # nothing judged


@pytest.mark.parametrize("name", CASES)
def test_reported_times_hold_the_peaks(harness, name):
    """the exact polynomial at the reported time is within the tolerance of the exact peak; no case is excluded for near-ties"""
    c = case(name)
    r = H.run(harness, **inputs(c))
    tol = L.tolerances(c["n_seg"], c["T"], c["coef"], c["src"], c["n_planes"], c["planes"])
    names = ("vpeak", "apeak", "jpeak", "cpeak")
    for b in np.flatnonzero(c["status"] == 0):
        n = int(c["n_seg"][b])
        for q in range(4 if c["planes"] is not None else 3):
            t = r["at"][b, q]
            assert 0.0 <= t <= c["t_total"][b]
            v = L.exact_value_at(n, c["T"][b], c["coef"][b], c["src"], q, t, None if c["planes"] is None else c["n_planes"][b],
                                 None if c["planes"] is None else c["planes"][b], r["c_where"][b])
            assert v is not None, (b, q)
            hi, lo = L.split(v)
            short = (c[names[q]][b] - hi) + (c[names[q] + "_lo"][b] - lo)      # exact peak minus the value at the reported time
            assert -tol[names[q]][b] * 1e-3 <= short <= tol[names[q]][b], (b, q, short / tol[names[q]][b] * L.TOL_UNITS)


def test_neutral_planes_touch_and_crossing(harness):
    c = case("synthetic_poly")
    r = H.run(harness, **inputs(c))
    neutral = [b for b in range(len(c["n_seg"])) if b not in (1, 3)]
    assert (r["cpeak"][neutral] == -1.0).all() and (r["at"][neutral, 3] == 0.0).all() and (r["c_where"][neutral] == 0).all()
    assert abs(r["cpeak"][3]) < 1e-15 and list(r["c_where"][3]) == [0, 1] and abs(r["at"][3, 3] - 0.25) < 1e-7   # touched
    assert r["cpeak"][1] == 1.5 and list(r["c_where"][1]) == [1, 0] and r["at"][1, 3] == 3.0                      # crossed at the end
    lim = dict(limits=(0.0, 0.0, 0.0, 0.0))
    v = H.run(harness, **inputs(c), **lim)["verdict"]
    assert (v[neutral] == 0).all() and v[1] == L.CORRIDOR
    v = H.run(harness, **inputs(c), limits=(0.0, 0.0, 0.0, 1.0))["verdict"]      # a margin of exactly 1: -1 > -1 is false
    assert (v[neutral] == 0).all() and v[3] == L.CORRIDOR
    v = H.run(harness, **inputs(c), limits=(0.0, 0.0, 0.0, 1.0 + 1e-12))["verdict"]
    assert (v == L.CORRIDOR).all()


def test_closed_forms(harness):
    """p = (s^5, 2 s^2, 3 - s) on [0, 2]: v = 80, a = 160, j = 240 at t = 2; the line and the constant"""
    for name in ("synthetic_poly", "synthetic_bez"):
        c = case(name)
        r = H.run(harness, **inputs(c))
        tol = 1e-12 if name.endswith("bez") else 0.0
        for f, want in (("vpeak", 80.0), ("apeak", 160.0), ("jpeak", 240.0)):
            assert abs(r[f][2] - want) <= tol * want, (name, f)
        assert (np.abs(r["at"][2, :3] - 2.0) <= tol).all()
        assert abs(r["vnorm"][2] - np.sqrt(80.0 ** 2 + 8.0 ** 2 + 1.0)) < 1e-12 * 81
        assert abs(r["vpeak"][1] - 2.0) <= 4 * tol and abs(r["vnorm"][1] - np.sqrt(5.25)) < 1e-15 * 4
        assert abs(r["apeak"][1]) < 1e-14 and r["vpeak"][0] == 0.0 and r["at"][0, 0] == 0.0
        assert abs(r["vpeak"][3] - 1.0) < 1e-15 and abs(r["at"][3, 0] - 0.25) < 1e-7      # between the samples 0.2 and 0.3
        assert r["gap"][2].max() == 0.0                                                  # n = 1


@pytest.mark.parametrize("name", PLAN_CASES)
def test_verdict_with_limits_beside_the_exact_peaks(harness, name):
    """limits at exact peak (1 +- 1e-6): the bit is clear / set (the tolerance is at most 3.4e-8 of a peak on these rows)"""
    c = case(name)
    B = len(c["n_seg"])
    for b in range(B):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in inputs(c).items()}
        for on_norm, names in ((0, ("vpeak", "apeak", "jpeak")), (1, ("vnorm", "anorm", "jnorm"))):
            peaks = [c[f][b] for f in names]
            cp = c["cpeak"][b]
            assert cp < 0 and min(peaks) > 0
            for sign, want in ((+1, 0), (-1, L.VEL | L.ACC | L.JERK | L.CORRIDOR)):
                limits = [p * (1 + sign * 1e-6) for p in peaks] + [-cp * (1 - sign * 1e-6)]
                r = H.run(harness, **one, limits=limits, on_norm=on_norm)
                assert r["verdict"][0] == want, (b, on_norm, sign)
                judged = [r[f][0] for f in names]
                assert abs(r["slowdown"][0] - L.slowdown(judged, limits)) <= 4 * L.U * r["slowdown"][0]
                assert (r["slowdown"][0] == 1.0) == (sign > 0)
            for q, bit in enumerate((L.VEL, L.ACC, L.JERK)):      # one limit at a time, the others not judged
                limits = [0.0, 0.0, 0.0, 0.0]
                limits[q] = peaks[q] * (1 - 1e-6)
                assert H.run(harness, **one, limits=limits, on_norm=on_norm)["verdict"][0] == bit


def test_best_is_the_cheapest_row_that_passes(harness):
    c = case("synthetic_free_poly")
    B = len(c["n_seg"])
    v = np.sort(c["vpeak"])
    mid = B // 2
    assert v[mid] - v[mid - 1] > 1e-6
    limits = (0.5 * (v[mid] + v[mid - 1]), 0.0, 0.0, 0.0)
    want_v = np.where(c["vpeak"] > limits[0], L.VEL, 0)
    rng = np.random.default_rng(2)
    cost = rng.uniform(1.0, 2.0, B)
    cheapest = np.flatnonzero(want_v == 0)[:2]
    cost[cheapest] = 0.5                                       # a tie: the smaller index
    cost[np.flatnonzero(want_v != 0)[0]] = 0.1                 # cheaper, but it fails
    rtn = np.zeros(B, np.int32)
    r = H.run(harness, **inputs(c), limits=limits, cost=cost, rtn=rtn)
    assert np.array_equal(r["verdict"], want_v)
    assert r["best"][0] == cheapest[0] == L.best_row(cost, want_v, rtn)
    rtn[cheapest[0]] = -4
    assert H.run(harness, **inputs(c), limits=limits, cost=cost, rtn=rtn)["best"][0] == cheapest[1]
    assert H.run(harness, **inputs(c), limits=limits, cost=cost)["best"][0] == cheapest[0]
    assert H.run(harness, **inputs(c), limits=(1e-9, 0.0, 0.0, 0.0), cost=cost)["best"][0] in (-1, 0)   # only the constant row can pass
    assert H.run(harness, **inputs(c), limits=limits, cost=np.full(B, np.nan))["best"][0] == -1


@pytest.mark.parametrize("name", CASES)
def test_sandwich_without_an_oracle(harness, name):
    """dense samples <= audited peak + tol, and audited peak <= the control polygon's largest magnitude + tol (convex hull)"""
    c = case(name)
    r = H.run(harness, **inputs(c))
    tol = L.tolerances(c["n_seg"], c["T"], c["coef"], c["src"], c["n_planes"], c["planes"])["seg_peak"]
    ok = np.flatnonzero(c["status"] == 0)
    L.sandwich(c["n_seg"], c["T"], c["coef"], c["src"], r["seg_peak"], tol, c["n_planes"], c["planes"], rows=ok)
    for b in ok:
        assert np.array_equal(r["seg_peak"][b, :int(c["n_seg"][b]), :3].max(0), [r["vpeak"][b], r["apeak"][b], r["jpeak"][b]])


def test_sampling_misses_the_jerk_peak(harness):
    """the motivating fact: on corridor_n20 phase 1 row 0 the sampler's loop (dt = 0.1, the end of a segment never visited) sees a
    jerk more than 10 % below the true peak, which sits at a segment end"""
    c = case("corridor_n20_p1_f64_poly")
    r = H.run(harness, **inputs(c))
    n = int(c["n_seg"][0])
    best = 0.0
    for i in range(n):
        T = c["T"][0, i]
        a = c["coef"][0, i].reshape(6, 3)
        tau = 0.0
        while tau < 1.0:
            s = tau * T
            best = max(best, np.abs(6 * a[3] + 24 * a[4] * s + 60 * a[5] * s * s).max())
            tau += 0.1 / T
    assert r["jpeak"][0] > 1.10 * best
    S = L.starts(c["T"][0], n)
    assert np.abs(S - r["at"][0, 2]).min() == 0.0


def test_independent_of_the_batch_a_row_is_in(harness):
    c = case("corridor_n8_p1_f64_bez")
    whole = H.run(harness, **inputs(c))
    perm = np.arange(len(c["n_seg"]))[::-1]
    p = {k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in inputs(c).items()}
    r = H.run(harness, **p)
    for f in L.ROW_FIELDS + ("at", "gap", "seg_peak", "c_where"):
        assert np.array_equal(r[f], whole[f][perm]), f
