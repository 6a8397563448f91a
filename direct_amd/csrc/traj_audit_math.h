// Arithmetic of direct_traj_audit_batch (include/direct_ddp.h, "continuous-time audit"): the exact maxima over closed
// segments of |p'|, |p''|, |p'''| per axis and as Euclidean norms, of the plane functions a x + b y + c z + d along the curve,
// the jumps across segment boundaries, and the verdict / slowdown of a row.  Plain C++ behind the qualifier macro of
// traj_eval_math.h: the kernels of traj_audit.h call these functions and g++ compiles the same header for the CPU test
// (tests/test_traj_audit_restatement.py).  Every multiply-add is an explicit fma() and contraction is switched off in
// every function, so the two compilers produce the same bits.
//
// Method.  Every quantity is the maximum of a polynomial f of degree <= 5 on [0, L], or of sum_d f_d^2; it is
// attained at 0, at L or at a root of the derivative g (degree M <= 4, for the squared norms sum_d f_d f_d' of degree <= 7).
// The roots of g are isolated by the DERIVATIVE LADDER: level m = 1 .. M holds the polynomial g^(M-m) / (M-m)! of degree m,
// whose sign changes on [0, L] lie one in each of the m pieces cut by the m - 1 points of the level below (the roots of its
// derivative: the polynomial is monotone on every piece).  A piece is halved kHalvings times keeping the half whose ends
// differ in sign; a piece without a sign change collapses onto its right end, a harmless extra cut.  So every level is an
// ascending list of exactly m points, every trip count is fixed and no lane waits for another's convergence.  The peak
// VALUE is always taken from the item's own Horner form at the candidate point (for norms from the three per-axis values):
// a critical point's position error enters the value to second order only.
#pragma once
#include "traj_eval_math.h"

#if defined(__clang__)
#define DIRECT_AUDIT_FP _Pragma("clang fp contract(off)")
#define DIRECT_AUDIT_LOOP _Pragma("nounroll")
#else
#define DIRECT_AUDIT_FP
#define DIRECT_AUDIT_LOOP
#endif

namespace direct {
namespace audit {

// Staged form of a segment: rec[m * 3 + d] = coefficient of x^m of axis d in the segment's own variable x in [0, L], then
// L, the seconds per unit of x, the factors sc_k that turn the k-th derivative in x into the k-th time derivative (k = 0..3),
// and the segment's start time S_i on the plan's clock.
constexpr int kL = 18, kTs = 19, kSc = 20, kS = 24;
constexpr int kRec = 25;        // doubles per record (odd: conflict-free 8-byte LDS reads at one record per lane)
constexpr int kHalvings = 30;   // a cut is placed to L 2^-30: 0.5 |f''| (L 2^-30)^2 <= 10 F 2^-60, below 0.1 u F
constexpr int kWs = 16;         // doubles per segment in the workspace, see W_* below
enum { W_V = 0, W_A = 1, W_J = 2, W_C = 3, W_TV = 4, W_TA = 5, W_TJ = 6, W_TC = 7, W_NV = 8, W_NA = 9, W_NJ = 10, W_PLANE = 11,
       W_G0 = 12, W_G1 = 13, W_G2 = 14, W_BAD = 15 };

#ifndef DIRECT_AUDIT_VEL  // the verdict bits of include/direct_ddp.h, for a build that does not see that header
#define DIRECT_AUDIT_VEL 1
#define DIRECT_AUDIT_ACC 2
#define DIRECT_AUDIT_JERK 4
#define DIRECT_AUDIT_CORRIDOR 8
#define DIRECT_AUDIT_INVALID 256
#endif

constexpr double binom(int n, int k) {
  double r = 1.0;
  for (int i = 1; i <= k; i++) r = r * (double)(n - k + i) / (double)i;  // exact: every prefix is a binomial coefficient
  return r;
}
constexpr double falling(int m, int k) {  // m! / (m - k)!
  double r = 1.0;
  for (int i = 0; i < k; i++) r = r * (double)(m - i);
  return r;
}

DIRECT_EVAL_HD int is_finite(double v) { return (v - v == 0.0) ? 1 : 0; }

// x = s in [0, T]: the getPolyCoeff() rows themselves
DIRECT_EVAL_HD void seg_from_poly(const double* a, double T, double S, double* rec) {
  eval::poly_table(a, rec);
  rec[kL] = T;
  rec[kTs] = 1.0;
  DIRECT_EVAL_UNROLL
  for (int k = 0; k < 4; k++) rec[kSc + k] = 1.0;
  rec[kS] = S;
}

// x = tau in [0, 1]: p(T tau) = T sum_j c_j B_j(tau) = T sum_m C(5, m) Delta^m c_0 tau^m; d^k/dt^k = T^-k d^k/dtau^k
DIRECT_EVAL_HD void seg_from_bez(const double* c, double T, double S, double* rec) {
  DIRECT_AUDIT_FP
  double tab[eval::kTab];
  eval::bez_table(c, T, tab);
  DIRECT_EVAL_UNROLL
  for (int d = 0; d < 3; d++) {
    DIRECT_EVAL_UNROLL
    for (int m = 0; m < 6; m++) rec[m * 3 + d] = binom(5, m) * tab[d * 6 + m];
  }
  const double inv = 1.0 / T;
  rec[kL] = 1.0;
  rec[kTs] = T;
  rec[kSc] = T;
  rec[kSc + 1] = 1.0;
  rec[kSc + 2] = inv;
  rec[kSc + 3] = inv * inv;
  rec[kS] = S;
}

template <int N>
DIRECT_EVAL_HD double horner(const double* q, double x) {
  double r = q[N];
  DIRECT_EVAL_UNROLL
  for (int i = N - 1; i >= 0; i--) r = fma(r, x, q[i]);
  return r;
}

// Level m of the ladder of p (degree M): in r[0 .. m-2] the cuts of level m - 1, out r[0 .. m-1] the cuts of level m, and on
// to level M.  The m halvings of a level are independent chains in one loop.
template <int M, int m>
DIRECT_EVAL_HD void ladder_level(const double* p, double L, double* r) {
  DIRECT_AUDIT_FP
  double q[m + 1], lo[m], hi[m];
  int pos[m];
  DIRECT_EVAL_UNROLL
  for (int i = 0; i <= m; i++) q[i] = binom(i + M - m, M - m) * p[i + M - m];
  DIRECT_EVAL_UNROLL
  for (int j = 0; j < m; j++) {
    lo[j] = j == 0 ? 0.0 : r[j - 1];
    hi[j] = j == m - 1 ? L : r[j];
    pos[j] = horner<m>(q, lo[j]) > 0.0;
  }
  DIRECT_AUDIT_LOOP
  for (int it = 0; it < kHalvings; it++) {
    DIRECT_EVAL_UNROLL
    for (int j = 0; j < m; j++) {
      const double mid = 0.5 * (lo[j] + hi[j]);
      const bool same = (horner<m>(q, mid) > 0.0) == (pos[j] != 0);
      lo[j] = same ? mid : lo[j];
      hi[j] = same ? hi[j] : mid;
    }
  }
  DIRECT_EVAL_UNROLL
  for (int j = 0; j < m; j++) r[j] = hi[j];
  if constexpr (m < M) ladder_level<M, m + 1>(p, L, r);
}

// r[0 .. M-1]: ascending points of [0, L] among which every sign change of p on [0, L] is found to L 2^-kHalvings
template <int M>
DIRECT_EVAL_HD void ladder(const double* p, double L, double* r) {
  ladder_level<M, 1>(p, L, r);
}

// the total order of the contract: the larger value, then the earlier time
DIRECT_EVAL_HD bool better(double v, double t, double bv, double bt) { return v > bv || (v == bv && t < bt); }
// ... then the earlier segment, then the smaller plane index
DIRECT_EVAL_HD bool better_c(double v, double t, double seg, double pl, double bv, double bt, double bseg, double bpl) {
  return v > bv || (v == bv && (t < bt || (t == bt && (seg < bseg || (seg == bseg && pl < bpl)))));
}

// max over x in [0, L] and the three axes of sc_K |d^K p_d / dx^K|, and its time on the plan's clock, into (bv, bt)
template <int K>
DIRECT_EVAL_HD void axis_peak(const double* rec, double& bv, double& bt) {
  DIRECT_AUDIT_FP
  constexpr int N = 5 - K, M = N - 1;
  const double L = rec[kL], ts = rec[kTs], sc = rec[kSc + K], S = rec[kS];
  bv = -1.0;
  bt = 0.0;
  DIRECT_EVAL_UNROLL
  for (int d = 0; d < 3; d++) {
    double c[N + 1], g[M + 1], r[M];
    DIRECT_EVAL_UNROLL
    for (int i = 0; i <= N; i++) c[i] = falling(i + K, K) * rec[(i + K) * 3 + d];
    DIRECT_EVAL_UNROLL
    for (int i = 0; i <= M; i++) g[i] = (double)(i + 1) * c[i + 1];
    ladder<M>(g, L, r);
    DIRECT_EVAL_UNROLL
    for (int q = 0; q < M + 2; q++) {
      const double x = q == 0 ? 0.0 : (q == M + 1 ? L : r[q - 1]);
      const double v = sc * fabs(horner<N>(c, x));
      const double xs = x * ts;
      const double t = S + xs;
      if (better(v, t, bv, bt)) {
        bv = v;
        bt = t;
      }
    }
  }
}

// max over x in [0, L] of sc_K |d^K p / dx^K|_2
template <int K>
DIRECT_EVAL_HD double norm_peak(const double* rec) {
  DIRECT_AUDIT_FP
  constexpr int N = 5 - K, M = 2 * N - 1;
  const double L = rec[kL], sc = rec[kSc + K];
  double c[3][N + 1], h[M + 1], r[M];
  DIRECT_EVAL_UNROLL
  for (int d = 0; d < 3; d++) {
    DIRECT_EVAL_UNROLL
    for (int i = 0; i <= N; i++) c[d][i] = falling(i + K, K) * rec[(i + K) * 3 + d];
  }
  DIRECT_EVAL_UNROLL
  for (int j = 0; j <= M; j++) {  // h = sum_d f_d f_d': only its sign changes are used
    double s = 0.0;
    DIRECT_EVAL_UNROLL
    for (int d = 0; d < 3; d++) {
      DIRECT_EVAL_UNROLL
      for (int i = 0; i <= N; i++) {
        const int l = j - i + 1;
        if (l >= 1 && l <= N) s = fma(c[d][i], (double)l * c[d][l], s);
      }
    }
    h[j] = s;
  }
  ladder<M>(h, L, r);
  double best = 0.0;
  DIRECT_EVAL_UNROLL
  for (int q = 0; q < M + 2; q++) {
    const double x = q == 0 ? 0.0 : (q == M + 1 ? L : r[q - 1]);
    const double f0 = horner<N>(c[0], x), f1 = horner<N>(c[1], x), f2 = horner<N>(c[2], x);
    const double n2 = fma(f2, f2, fma(f1, f1, f0 * f0));
    best = n2 > best ? n2 : best;
  }
  return sc * sqrt(best);
}

// max over x in [0, L] of a x + b y + c z + d at the curve, and its time: the earliest on a tie
DIRECT_EVAL_HD void plane_peak(const double* rec, double a, double b, double c, double d, double& bv, double& bt) {
  DIRECT_AUDIT_FP
  const double L = rec[kL], ts = rec[kTs], sc = rec[kSc], S = rec[kS];
  double f[6], g[5], r[4];
  DIRECT_EVAL_UNROLL
  for (int m = 0; m < 6; m++) f[m] = fma(c, rec[m * 3 + 2], fma(b, rec[m * 3 + 1], a * rec[m * 3]));
  DIRECT_EVAL_UNROLL
  for (int i = 0; i < 5; i++) g[i] = (double)(i + 1) * f[i + 1];
  ladder<4>(g, L, r);
  DIRECT_EVAL_UNROLL
  for (int q = 0; q < 6; q++) {
    const double x = q == 0 ? 0.0 : (q == 5 ? L : r[q - 1]);
    const double v = fma(sc, horner<5>(f, x), d);
    const double xs = x * ts;
    const double t = S + xs;
    if (q == 0 || better(v, t, bv, bt)) {
      bv = v;
      bt = t;
    }
  }
}

// the jumps of position, velocity and acceleration (max over the axes) from the end of segment `prev` to the start of `cur`
DIRECT_EVAL_HD void gap3(const double* prev, const double* cur, double* gap) {
  DIRECT_AUDIT_FP
  const double L = prev[kL];
  gap[0] = gap[1] = gap[2] = 0.0;
  DIRECT_EVAL_UNROLL
  for (int d = 0; d < 3; d++) {
    double c0[6], c1[5], c2[4];
    DIRECT_EVAL_UNROLL
    for (int i = 0; i < 6; i++) c0[i] = prev[i * 3 + d];
    DIRECT_EVAL_UNROLL
    for (int i = 0; i < 5; i++) c1[i] = falling(i + 1, 1) * prev[(i + 1) * 3 + d];
    DIRECT_EVAL_UNROLL
    for (int i = 0; i < 4; i++) c2[i] = falling(i + 2, 2) * prev[(i + 2) * 3 + d];
    const double e0 = prev[kSc] * horner<5>(c0, L), e1 = prev[kSc + 1] * horner<4>(c1, L), e2 = prev[kSc + 2] * horner<3>(c2, L);
    const double s0 = cur[kSc] * cur[d], s1 = cur[kSc + 1] * cur[3 + d], s2 = cur[kSc + 2] * (2.0 * cur[6 + d]);
    gap[0] = fmax(gap[0], fabs(e0 - s0));
    gap[1] = fmax(gap[1], fabs(e1 - s1));
    gap[2] = fmax(gap[2], fabs(e2 - s2));
  }
}

struct Limits {
  double max_vel, max_acc, max_jerk, clearance;
  int on_norm, planes;
};

// items 6 and 7 of the contract from the judged peaks (per axis or norm), in double
DIRECT_EVAL_HD int verdict_of(const Limits& l, double v, double a, double j, double c) {
  DIRECT_AUDIT_FP
  int w = 0;
  if (l.max_vel > 0.0 && v > l.max_vel) w |= DIRECT_AUDIT_VEL;
  if (l.max_acc > 0.0 && a > l.max_acc) w |= DIRECT_AUDIT_ACC;
  if (l.max_jerk > 0.0 && j > l.max_jerk) w |= DIRECT_AUDIT_JERK;
  if (l.planes && c > -l.clearance) w |= DIRECT_AUDIT_CORRIDOR;
  return w;
}
DIRECT_EVAL_HD double slowdown_of(const Limits& l, double v, double a, double j) {
  DIRECT_AUDIT_FP
  double s = 1.0;
  if (l.max_vel > 0.0) s = fmax(s, v / l.max_vel);
  if (l.max_acc > 0.0) s = fmax(s, sqrt(a / l.max_acc));
  if (l.max_jerk > 0.0) s = fmax(s, cbrt(j / l.max_jerk));
  return s;
}

// One segment's workspace record from its staged form (planes excluded): w[W_*].  norms: also the three Euclidean peaks.
DIRECT_EVAL_HD void segment_items(const double* rec, const double* prev, int norms, double* w) {
  w[W_NV] = w[W_NA] = w[W_NJ] = 0.0;
  if (norms) {  // the deepest ladders first, while nothing else of the record is live
    w[W_NV] = norm_peak<1>(rec);
    w[W_NA] = norm_peak<2>(rec);
    w[W_NJ] = norm_peak<3>(rec);
  }
  axis_peak<1>(rec, w[W_V], w[W_TV]);
  axis_peak<2>(rec, w[W_A], w[W_TA]);
  axis_peak<3>(rec, w[W_J], w[W_TJ]);
  w[W_G0] = w[W_G1] = w[W_G2] = 0.0;
  if (prev) gap3(prev, rec, w + W_G0);
  w[W_C] = 0.0;
  w[W_TC] = 0.0;
  w[W_PLANE] = 0.0;
}

// A row's reduction over its segments' workspace records.  add() and merge() apply the total order, so the result does not
// depend on how the segments are spread over lanes (the kernel) or visited (the CPU harness: add() in turn).
struct RowAcc {
  double v[3], t[3], c, tc, cseg, cpl, nrm[3], gap[3];
  int bad;
};
DIRECT_EVAL_HD void row_init(RowAcc& A) {
  DIRECT_EVAL_UNROLL
  for (int k = 0; k < 3; k++) {
    A.v[k] = -1.0;
    A.t[k] = 0.0;
    A.nrm[k] = 0.0;
    A.gap[k] = 0.0;
  }
  A.c = -INFINITY;
  A.tc = A.cseg = A.cpl = 0.0;
  A.bad = 0;
}
DIRECT_EVAL_HD void row_merge(RowAcc& A, const RowAcc& B) {
  DIRECT_EVAL_UNROLL
  for (int k = 0; k < 3; k++) {
    if (better(B.v[k], B.t[k], A.v[k], A.t[k])) {
      A.v[k] = B.v[k];
      A.t[k] = B.t[k];
    }
    A.nrm[k] = B.nrm[k] > A.nrm[k] ? B.nrm[k] : A.nrm[k];
    A.gap[k] = B.gap[k] > A.gap[k] ? B.gap[k] : A.gap[k];
  }
  if (better_c(B.c, B.tc, B.cseg, B.cpl, A.c, A.tc, A.cseg, A.cpl)) {
    A.c = B.c;
    A.tc = B.tc;
    A.cseg = B.cseg;
    A.cpl = B.cpl;
  }
  A.bad |= B.bad;
}
DIRECT_EVAL_HD void row_add(RowAcc& A, int i, const double* w, int planes) {
  RowAcc B;
  DIRECT_EVAL_UNROLL
  for (int k = 0; k < 3; k++) {
    B.v[k] = w[W_V + k];
    B.t[k] = w[W_TV + k];
    B.nrm[k] = w[W_NV + k];
    B.gap[k] = w[W_G0 + k];
  }
  B.c = planes ? w[W_C] : -INFINITY;
  B.tc = w[W_TC];
  B.cseg = (double)i;
  B.cpl = w[W_PLANE];
  B.bad = w[W_BAD] != 0.0;
  row_merge(A, B);
}

struct RowOut {
  double peak[7];  // vpeak, apeak, jpeak, vnorm, anorm, jnorm, cpeak
  double at[4], gap[3], slowdown;
  int c_where[2], verdict;
};
DIRECT_EVAL_HD void row_finish(const RowAcc& A, const Limits& l, RowOut& o) {
  DIRECT_EVAL_UNROLL
  for (int k = 0; k < 3; k++) {
    o.peak[k] = A.v[k];
    o.peak[3 + k] = A.nrm[k];
    o.at[k] = A.t[k];
    o.gap[k] = A.gap[k];
  }
  o.peak[6] = l.planes ? A.c : 0.0;
  o.at[3] = l.planes ? A.tc : 0.0;
  o.c_where[0] = l.planes ? (int)A.cseg : 0;
  o.c_where[1] = l.planes ? (int)A.cpl : 0;
  const int q = l.on_norm ? 3 : 0;
  o.verdict = verdict_of(l, o.peak[q], o.peak[q + 1], o.peak[q + 2], o.peak[6]);
  o.slowdown = slowdown_of(l, o.peak[q], o.peak[q + 1], o.peak[q + 2]);
}

// A segment's plane items folded into its record in ascending plane order (the smaller index wins a tie)
DIRECT_EVAL_HD void segment_plane(double* w, int k, double v, double t) {
  if (k == 0 || better(v, t, w[W_C], w[W_TC])) {
    w[W_C] = v;
    w[W_TC] = t;
    w[W_PLANE] = (double)k;
  }
}

}  // namespace audit
}  // namespace direct
