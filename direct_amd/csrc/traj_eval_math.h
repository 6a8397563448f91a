// Per-row and per-query arithmetic of direct_traj_eval_batch (include/direct_ddp.h, "trajectory evaluation"): segment
// start times, segment choice and the evaluation of position .. snap from one segment's Bezier control points or monomial
// coefficients.  Plain C++ behind a qualifier macro: the kernels of traj_eval.h call these functions, and g++ compiles the
// same header for the CPU test (tests/test_traj_eval_restatement.py).  Every multiply-add is an explicit fma() and nothing
// else can be contracted, so the two compilers produce the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DIRECT_EVAL_HD __host__ __device__ __forceinline__
#else
#define DIRECT_EVAL_HD inline
#endif
#if defined(__clang__)
#define DIRECT_EVAL_UNROLL _Pragma("unroll")  // constant indices everywhere: the small arrays below stay in registers
#else
#define DIRECT_EVAL_UNROLL
#endif

namespace direct {
namespace eval {

constexpr int kTab = 22;  // doubles per staged segment: 18 coefficients, then T, 20 / T, 60 / T^2, 120 / T^3 (Bezier only)

// S[0..n] = 0, T_0, T_0 + T_1, ... summed left to right in double (numpy.cumsum).  Returns 0 when the row is invalid: n outside
// [1, nmax] or one of its first n durations not a finite number > 0.
template <typename St>
DIRECT_EVAL_HD int row_starts(const St* __restrict__ T, int n, int nmax, double* __restrict__ S) {
  if (n < 1 || n > nmax) return 0;
  int ok = 1;
  double s = 0.0;
  S[0] = 0.0;
#if defined(__clang__)
#pragma unroll 8
#endif
  for (int i = 0; i < n; i++) {  // no early exit: the loads of an unrolled block are issued together
    const double Ti = (double)T[i];
    ok &= (Ti > 0.0 && Ti <= 1.7976931348623157e308) ? 1 : 0;
    s = s + Ti;
    S[i + 1] = s;
  }
  return ok;
}

// t0 + j * dt with the product rounded before the sum (t0 + numpy.arange(m) * dt)
DIRECT_EVAL_HD double grid_time(double t0, int j, double dt) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double p = (double)j * dt;
  return t0 + p;
}

// Segment of time t on a valid row: seg = the largest i in [0, n-1] with S[i] <= t_c, t_c = min(max(t, 0), S[n]), and
// s = t_c - S[seg].  A NaN t gives seg = -1 and s = NaN.  The halving loop runs the same number of steps in every lane of a
// wave (it depends on n only).
struct Loc {
  int seg;
  double s;
};
DIRECT_EVAL_HD Loc locate(const double* S, int n, double t) {
  if (t != t) return Loc{-1, t};
  const double c = fmin(fmax(t, 0.0), S[n]);
  int base = 0, len = n;
  while (len > 1) {
    const int half = len >> 1;
    base = (S[base + half] <= c) ? base + half : base;
    len -= half;
  }
  return Loc{base, c - S[base]};
}

// Staged form of a segment given by getBezCoeff() control points c[d * 6 + j] (time-scaled) and its duration: per axis the
// forward differences D_k = Delta^k c_0 (k = 0..5), then T and the derivative scales.
DIRECT_EVAL_HD void bez_table(const double* c, double T, double* tab) {
  DIRECT_EVAL_UNROLL
  for (int d = 0; d < 3; d++) {
    double w[6];
    DIRECT_EVAL_UNROLL
    for (int j = 0; j < 6; j++) w[j] = c[d * 6 + j];
    tab[d * 6] = w[0];
    DIRECT_EVAL_UNROLL
    for (int lvl = 1; lvl < 6; lvl++) {
      DIRECT_EVAL_UNROLL
      for (int j = 0; j + lvl < 6; j++) w[j] = w[j + 1] - w[j];
      tab[d * 6 + lvl] = w[0];
    }
  }
  const double inv = 1.0 / T;
  tab[18] = T;
  tab[19] = 20.0 * inv;
  tab[20] = (60.0 * inv) * inv;
  tab[21] = ((120.0 * inv) * inv) * inv;
}

// Derivatives k = 0..4 at normalised time tau into out[k * 3 + d].  The k-th one is T^(1-k) 5!/(5-k)! times the Bernstein
// sum of degree 5-k over the k-th differences, evaluated in the monomial basis: sum_i C(5-k, i) D_(k+i) tau^i (the same
// polynomial; k_sample uses this form for k <= 2), by Horner with the binomial ratios C(n, i+1) / C(n, i) riding on tau.
DIRECT_EVAL_HD void eval_bez(const double* tab, double tau, double* out) {
  const double p5[5] = {5.0 * tau, 2.0 * tau, tau, 0.5 * tau, 0.2 * tau};
  const double p4[4] = {4.0 * tau, 1.5 * tau, (2.0 / 3.0) * tau, 0.25 * tau};
  const double p3[3] = {3.0 * tau, tau, (1.0 / 3.0) * tau};
  const double p2[2] = {2.0 * tau, 0.5 * tau};
  const double sc[5] = {tab[18], 5.0, tab[19], tab[20], tab[21]};
  DIRECT_EVAL_UNROLL
  for (int d = 0; d < 3; d++) {
    const double* D = tab + d * 6;
    double r0 = D[5], r1 = D[5], r2 = D[5], r3 = D[5];
    DIRECT_EVAL_UNROLL
    for (int q = 4; q >= 0; q--) r0 = fma(r0, p5[q], D[q]);
    DIRECT_EVAL_UNROLL
    for (int q = 3; q >= 0; q--) r1 = fma(r1, p4[q], D[q + 1]);
    DIRECT_EVAL_UNROLL
    for (int q = 2; q >= 0; q--) r2 = fma(r2, p3[q], D[q + 2]);
    DIRECT_EVAL_UNROLL
    for (int q = 1; q >= 0; q--) r3 = fma(r3, p2[q], D[q + 3]);
    const double r4 = fma(D[5], tau, D[4]);
    out[d] = sc[0] * r0;
    out[3 + d] = sc[1] * r1;
    out[6 + d] = sc[2] * r2;
    out[9 + d] = sc[3] * r3;
    out[12 + d] = sc[4] * r4;
  }
}

// Normalised time of a Bezier segment from s = t_c - S_i: min(s / T_i, 1)
DIRECT_EVAL_HD double bez_tau(double s, const double* tab) { return fmin(s / tab[18], 1.0); }

// Staged form of a segment given by getPolyCoeff() rows a[m * 3 + d]: the coefficients themselves (tab[18..21] unused)
DIRECT_EVAL_HD void poly_table(const double* a, double* tab) {
  DIRECT_EVAL_UNROLL
  for (int q = 0; q < 18; q++) tab[q] = a[q];
}

// Derivatives k = 0..4 of sum_m a_m s^m, a_m = tab[m * 3 + d] (getPolyCoeff() rows), at s = t_c - S_i, into out[k * 3 + d]
DIRECT_EVAL_HD void eval_poly(const double* tab, double s, double* out) {
  DIRECT_EVAL_UNROLL
  for (int d = 0; d < 3; d++) {
    const double a0 = tab[d], a1 = tab[3 + d], a2 = tab[6 + d], a3 = tab[9 + d], a4 = tab[12 + d], a5 = tab[15 + d];
    out[d] = fma(fma(fma(fma(fma(a5, s, a4), s, a3), s, a2), s, a1), s, a0);
    out[3 + d] = fma(fma(fma(fma(5.0 * a5, s, 4.0 * a4), s, 3.0 * a3), s, 2.0 * a2), s, a1);
    out[6 + d] = fma(fma(fma(20.0 * a5, s, 12.0 * a4), s, 6.0 * a3), s, 2.0 * a2);
    out[9 + d] = fma(fma(60.0 * a5, s, 24.0 * a4), s, 6.0 * a3);
    out[12 + d] = fma(120.0 * a5, s, 24.0 * a4);
  }
}

}  // namespace eval
}  // namespace direct
