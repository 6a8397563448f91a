"""The contract of direct_traj_eval_batch (include/direct_ddp.h) on the CPU: its NumPy restatement (tests/traj_eval_lib.py)
against the committed sampler and solver goldens and closed forms, and the per-query arithmetic the kernels run
(direct_amd/csrc/traj_eval_math.h, compiled here by g++) against the restatement."""
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import traj_eval_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE_CASES = ("corridor_n8", "free_n5", "config1_n50")
SOLVE_CASES = ("corridor_n8", "corridor_n20", "free_n5", "free_n6_tp1", "config1_n50")


def golden(name):
    return np.load(os.path.join(helpers.GOLDEN_DIR, name + ".npz"))


@pytest.mark.parametrize("case", SAMPLE_CASES)
def test_sampler_goldens_at_their_absolute_times(case):
    """Every stored sample of the sampler's loop (time restarting in each segment) is the plan at S_i + tau T_i."""
    g = golden("sample_" + case)
    t = L.sampler_times(g["n_seg"], g["T"], float(g["dt"]), int(g["capacity"]))
    r = L.evaluate(g["n_seg"], g["T"], bez=g["bez"], times=np.nan_to_num(t))
    for b in range(len(g["n_seg"])):
        k = min(int(g["count"][b]), int(g["capacity"]))
        assert np.isnan(t[b, k:]).all() and not np.isnan(t[b, :k]).any()
        for f in ("pos", "vel", "acc"):
            assert helpers.rel(r[f][b, :k], g[f][b, :k]) < 1e-12, (b, f)


@pytest.mark.parametrize("case", SOLVE_CASES)
@pytest.mark.parametrize("phase", ["p0_", "p1_"])
def test_jerk_cost_identity(case, phase):
    """getJerkCost() is the integral of |jerk|^2 over the trajectory: a 3-point Gauss-Legendre rule per segment is exact."""
    g = golden(case)
    t, w = L.gauss_times(g["n_seg"], g[phase + "T"])
    for src, tol in (("poly", 1e-12), ("bez", 1e-9)):
        r = L.evaluate(g["n_seg"], g[phase + "T"], times=t, **{src: g[phase + src]})
        assert (r["status"] == 0).all()
        assert np.abs(L.jerk_cost(r["jerk"], w) / g[phase + "jerk_cost"] - 1).max() < tol, src


@pytest.mark.parametrize("case", SOLVE_CASES)
def test_start_state_and_continuity(case):
    """state at t = 0 is x0 (the solve's own start); [p, v, a] are continuous across every interior S_i."""
    g = golden(case)
    n_seg, T = g["n_seg"], g["p1_T"]
    r = L.evaluate(n_seg, T, poly=g["p1_poly"], times=np.zeros((len(n_seg), 1)))
    assert np.array_equal(r["state"][:, 0], g["x0"])
    rb = L.evaluate(n_seg, T, bez=g["p1_bez"], times=np.zeros((len(n_seg), 1)))
    assert helpers.rel(rb["state"][:, 0], g["x0"]) < 1e-12
    for b in range(len(n_seg)):
        n = int(n_seg[b])
        S = L.starts(T[b], n)
        at = L.evaluate(n_seg[b:b + 1], T[b:b + 1], poly=g["p1_poly"][b:b + 1], times=S[None, 1:n])
        assert (at["seg"][0] == np.arange(1, n)).all()
        end = L.poly_derivs(g["p1_poly"][b, :n - 1].reshape(-1, 6, 3), T[b, :n - 1])
        for k in range(3):
            assert helpers.rel(at[L.NAMES[k]][0], end[k]) < 1e-12, (b, k)


def test_boundary_rule_clamping_nan_and_invalid_rows():
    g = golden("corridor_n8")
    n_seg, T, bez = g["n_seg"], g["p1_T"], g["p1_bez"]
    S = L.starts(T[0], int(n_seg[0]))
    n = int(n_seg[0])
    t = np.array([S[3], -1.0, 0.0, S[n] + 5.0, S[n], np.nan, np.nextafter(S[3], 0.0)])
    r = L.evaluate(n_seg[:1], T[:1], bez=bez[:1], times=t[None])
    assert list(r["seg"][0]) == [3, 0, 0, n - 1, n - 1, -1, 2]
    c = bez[0].reshape(-1, 3, 6)
    start3 = L.bez_derivs(c[3:4], T[0, 3:4], np.zeros(1))
    end2 = L.bez_derivs(c[2:3], T[0, 2:3], np.ones(1))
    assert np.array_equal(r["jerk"][0, 0], start3[3, 0]) and np.array_equal(r["snap"][0, 0], start3[4, 0])
    assert np.abs(start3[3, 0] - end2[3, 0]).max() > 1e-6       # jerk jumps there: the later segment's is the one returned
    for f in L.NAMES:
        assert np.array_equal(r[f][0, 1], r[f][0, 2]) and np.array_equal(r[f][0, 3], r[f][0, 4])
        assert np.isnan(r[f][0, 5]).all()
    assert r["t_total"][0] == S[n]
    # invalid rows: n outside [1, n_seg_max], a duration 0, negative, inf or NaN; the valid row is unaffected
    B = 7
    nn = np.repeat(n_seg[:1], B)
    TT = np.repeat(T[:1], B, 0)
    nn[1], nn[2] = 0, T.shape[1] + 1
    TT[3, 1], TT[4, 2], TT[5, 0], TT[6, n - 1] = 0.0, -0.5, np.inf, np.nan
    TT[0, n:] = -1.0            # entries past n_seg are never read
    rr = L.evaluate(nn, TT, bez=np.repeat(bez[:1], B, 0), times=np.repeat(t[None], B, 0), n_query=[7, 7, 7, 7, 7, 5, 7])
    assert list(rr["status"]) == [0, -1, -1, -1, -1, -1, -1]
    assert (rr["seg"][1:5] == -1).all() and (rr["seg"][5, :5] == -1).all() and (rr["seg"][5, 5:] == 0).all()
    for f in L.NAMES + ("state", "t_total"):
        assert (rr[f][1:] == 0).all()
        assert np.array_equal(rr[f][0], r[f][0], equal_nan=True)


def test_single_quintic_closed_forms():
    """p(s) = s^5 on x, 2 s^2 on y, 3 - s on z over one segment of T = 2, from poly and from bez."""
    T = 2.0
    poly = np.zeros((1, 1, 6, 3))
    poly[0, 0, 5, 0], poly[0, 0, 2, 1], poly[0, 0, 0, 2], poly[0, 0, 1, 2] = 1.0, 2.0, 3.0, -1.0
    # the same curve as time-scaled Bezier control points: p(T tau) = T sum_j c_j B_j(tau)
    M = np.array([[np.prod([(j - q) / (5 - q) for q in range(m)]) if j >= m else 0.0 for m in range(6)] for j in range(6)])
    a_tau = poly[0, 0] * (T ** np.arange(6))[:, None]             # coefficients in tau
    bez = (M @ a_tau).T.reshape(1, 1, 18) / T                     # c_j = sum_m C(j,m)/C(5,m) a_m / T
    s = np.array([0.0, 0.3, 1.0, 1.7, 2.0])
    want = {"pos": np.stack([s ** 5, 2 * s ** 2, 3 - s], 1), "vel": np.stack([5 * s ** 4, 4 * s, -np.ones_like(s)], 1),
            "acc": np.stack([20 * s ** 3, 4 + 0 * s, 0 * s], 1), "jerk": np.stack([60 * s ** 2, 0 * s, 0 * s], 1),
            "snap": np.stack([120 * s, 0 * s, 0 * s], 1)}
    for src in ({"poly": poly.reshape(1, 1, 18)}, {"bez": bez}):
        r = L.evaluate([1], [[T]], times=s[None], **src)
        for f in L.NAMES:
            assert np.abs(r[f][0] - want[f]).max() < 1e-12 * max(1.0, np.abs(want[f]).max()), (list(src), f)


def test_grid_times_are_t0_plus_arange_times_dt():
    g = golden("free_n5")
    r = L.evaluate(g["n_seg"], g["p1_T"], poly=g["p1_poly"], t0=-0.3, dt=0.07, m=200, n_query=[200, 17, 0])
    e = L.evaluate(g["n_seg"], g["p1_T"], poly=g["p1_poly"], times=np.tile(-0.3 + np.arange(200) * 0.07, (3, 1)),
                   n_query=[200, 17, 0])
    for f in L.NAMES + ("seg",):
        assert np.array_equal(r[f], e[f])
    assert (r["seg"][1, 17:] == 0).all() and (r["pos"][2] == 0).all()


HARNESS = r'''
#include <cstdio>
#include <vector>
#include "traj_eval_math.h"
using namespace direct::eval;
// in: int32 B, nmax, m, poly, grid, pad; float64 t0, dt; int32 n_seg[B]; float64 T[B][nmax], coef[B][nmax][18], t[B][m]
// out: per row float64 status, t_total, then per query seg and 15 values - the kernels' sequence of calls
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  int h[6]; double g[2];
  if (fread(h, 4, 6, f) != 6 || fread(g, 8, 2, f) != 2) return 1;
  const int B = h[0], nm = h[1], m = h[2], poly = h[3], grid = h[4];
  std::vector<int> n_seg(B); std::vector<double> T((size_t)B * nm), coef((size_t)B * nm * 18), t((size_t)B * m);
  if (fread(n_seg.data(), 4, B, f) != (size_t)B || fread(T.data(), 8, T.size(), f) != T.size() ||
      fread(coef.data(), 8, coef.size(), f) != coef.size() || fread(t.data(), 8, t.size(), f) != t.size()) return 1;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  std::vector<double> S(nm + 1);
  for (int b = 0; b < B; b++) {
    const int ok = row_starts(&T[(size_t)b * nm], n_seg[b], nm, S.data());
    const double head[2] = {ok ? 0.0 : -1.0, ok ? S[n_seg[b]] : 0.0};
    fwrite(head, 8, 2, o);
    for (int q = 0; q < m; q++) {
      double rec[16] = {-1.0};
      if (ok) {
        const double tq = grid ? grid_time(g[0], q, g[1]) : t[(size_t)b * m + q];
        const Loc L = locate(S.data(), n_seg[b], tq);
        rec[0] = L.seg;
        if (L.seg < 0) {
          for (int j = 1; j < 16; j++) rec[j] = L.s;
        } else {
          double tab[kTab];
          const double* c = &coef[((size_t)b * nm + L.seg) * 18];
          if (poly) { poly_table(c, tab); eval_poly(tab, L.s, rec + 1); }
          else { bez_table(c, T[(size_t)b * nm + L.seg], tab); eval_bez(tab, bez_tau(L.s, tab), rec + 1); }
        }
      }
      fwrite(rec, 8, 16, o);
    }
  }
  fclose(o);
  return 0;
}
'''


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_math")
    (d / "h.cpp").write_text(HARNESS)
    exe = d / "h"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "direct_amd", "csrc"),
                           str(d / "h.cpp"), "-o", str(exe)])
    return d, exe


def run_harness(harness, n_seg, T, coef, poly, times=None, t0=0.0, dt=0.0, m=None):
    d, exe = harness
    B, nm = T.shape
    m = times.shape[1] if times is not None else m
    with open(d / "in.bin", "wb") as f:
        np.array([B, nm, m, int(poly), int(times is None), 0], np.int32).tofile(f)
        np.array([t0, dt], np.float64).tofile(f)
        np.asarray(n_seg, np.int32).tofile(f)
        np.asarray(T, np.float64).tofile(f)
        np.asarray(coef, np.float64).tofile(f)
        (np.zeros((B, m)) if times is None else np.asarray(times, np.float64)).tofile(f)
    subprocess.check_call([str(exe), str(d / "in.bin"), str(d / "out.bin")])
    out = np.fromfile(d / "out.bin", np.float64)
    res, pos = dict(status=np.zeros(B, np.int32), t_total=np.zeros(B), seg=np.zeros((B, m), np.int32)), 0
    vals = np.zeros((B, m, 15))
    for b in range(B):
        res["status"][b], res["t_total"][b] = out[pos], out[pos + 1]
        rec = out[pos + 2:pos + 2 + 16 * m].reshape(m, 16)
        res["seg"][b], vals[b] = rec[:, 0], rec[:, 1:]
        pos += 2 + 16 * m
    for k, name in enumerate(L.NAMES):
        res[name] = vals[:, :, 3 * k:3 * k + 3]
    return res


def compare(c, r, tol_pva=1e-12, tol_js=1e-9):
    assert (c["status"] == r["status"]).all() and (c["seg"] == r["seg"]).all()
    assert np.array_equal(c["t_total"], r["t_total"])
    for k, name in enumerate(L.NAMES):
        tol = tol_pva if k < 3 else tol_js
        for b in range(len(c["status"])):
            a, e = c[name][b], r[name][b]
            nan = np.isnan(e)
            assert np.array_equal(np.isnan(a), nan)
            if (~nan).any():
                assert np.abs(a - e)[~nan].max() <= tol * (np.abs(e[~nan]).max() + 1e-300), (b, name)


@pytest.mark.parametrize("src", ["bez", "poly"])
def test_compiled_math_matches_the_restatement(harness, src):
    rng = np.random.default_rng(5)
    for case in SOLVE_CASES:
        g = golden(case)
        n_seg, T, coef = g["n_seg"].copy(), g["p1_T"].copy(), g["p1_" + src]
        B, nm = T.shape
        S_end = np.array([L.starts(T[b], int(n_seg[b]))[-1] for b in range(B)])
        times = rng.uniform(-0.5, S_end.max() + 0.5, (B, 300))
        for b in range(B):   # every segment boundary and its neighbours, and a NaN
            S = L.starts(T[b], int(n_seg[b]))
            k = len(S)
            times[b, :k], times[b, k:2 * k], times[b, 2 * k:3 * k] = S, np.nextafter(S, -1.0), np.nextafter(S, 1e9)
            times[b, 3 * k] = np.nan
        n_bad = n_seg.copy()
        n_bad[0] = 0
        for nn in (n_seg, n_bad):
            c = run_harness(harness, nn, T, coef, src == "poly", times=times)
            compare(c, L.evaluate(nn, T, times=times, **{src: coef}))
        c = run_harness(harness, n_seg, T, coef, src == "poly", t0=-0.25, dt=0.0173, m=700)
        compare(c, L.evaluate(n_seg, T, t0=-0.25, dt=0.0173, m=700, **{src: coef}))
