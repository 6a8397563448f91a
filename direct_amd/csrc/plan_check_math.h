// Arithmetic of direct_cluster_plan_check_batch (include/direct_cluster.h, "plans against the resident map"): a segment's control
// points in metres, one de Casteljau halving, the voxel-index box of six points, the times of leaves and subtrees, and the descent
// that finds a segment's first blocked judged leaf.  Plain C++ behind a qualifier macro: the kernels of plan_check.h call these
// functions, and g++ compiles the same header for the CPU tests (tests/plan_check_harness.py).
//
// Everything is double, written with plain * and + and no fma(), and contraction is off (the pragma below under clang; g++ gets
// -ffp-contract=off from the harness): the NumPy restatement performs the same operations and must get the same bits.
//
// Why the descent may prune: (a + b) * 0.5 of two doubles in [m, M] lies in [m, M] because rounding is monotone,
// so the six points of a child lie in the per-axis range of its parent's and - every step of box_of() being monotone - the child's
// index box lies inside the parent's.  A subtree (d, k) ends at S + ((k + 1) * 2^-d) * T, which is bit for bit the end of its last
// leaf ((k + 1) * 2^-d is exact and the same number).  Hence an unblocked node has no blocked leaf below it, and a node that ends
// at or before t_from has no judged leaf below it.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DIRECT_PLANCHECK_HD __host__ __device__ __forceinline__
#else
#define DIRECT_PLANCHECK_HD inline
#endif
#if defined(__clang__)
#define DIRECT_PLANCHECK_NO_CONTRACT _Pragma("clang fp contract(off)")
#define DIRECT_PLANCHECK_UNROLL _Pragma("unroll")
#else
#define DIRECT_PLANCHECK_NO_CONTRACT
#define DIRECT_PLANCHECK_UNROLL
#endif

namespace direct {
namespace plancheck {

constexpr int kMaxDepth = 12;
constexpr double kMaxCoord = 1e300;  // a control point in metres beyond this (or not a number) makes its row invalid
constexpr int kNone = -1;            // no blocked judged leaf
constexpr int kBadCoef = -2;         // the segment's control points are not all finite and within kMaxCoord
constexpr int kOpen = -3;            // descend() ran out of its budget of nodes

struct Grid {
  double lower[3];
  double inv, margin;
  int size[3];
  int outside_blocks;
};

// Control points P[a * 6 + j] in metres from getBezCoeff() control points c[a * 6 + j]: P_j = T * c_j.  Returns 0 when one of
// them is not usable (see kMaxCoord; a non-finite coefficient always gives one).
template <typename St>
DIRECT_PLANCHECK_HD int ctrl_from_bez(const St* __restrict__ c, double T, double* __restrict__ P) {
  DIRECT_PLANCHECK_NO_CONTRACT
  int ok = 1;
  DIRECT_PLANCHECK_UNROLL
  for (int q = 0; q < 18; q++) {
    P[q] = T * (double)c[q];
    ok &= fabs(P[q]) <= kMaxCoord ? 1 : 0;
  }
  return ok;
}

// ... from getPolyCoeff() rows a[m * 3 + d] (coefficient of s^m): b_j = sum_{m <= j} w[j][m] * (a_m * T^m), ascending m,
// w[j][m] = (double)C(j, m) / (double)C(5, m), T^m by repeated multiplication from 1.
template <typename St>
DIRECT_PLANCHECK_HD int ctrl_from_poly(const St* __restrict__ a, double T, double* __restrict__ P) {
  DIRECT_PLANCHECK_NO_CONTRACT
  const double binom[6][6] = {{1, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 0}, {1, 2, 1, 0, 0, 0},
                              {1, 3, 3, 1, 0, 0}, {1, 4, 6, 4, 1, 0}, {1, 5, 10, 10, 5, 1}};
  double Tm[6];
  Tm[0] = 1.0;
  DIRECT_PLANCHECK_UNROLL
  for (int m = 1; m < 6; m++) Tm[m] = Tm[m - 1] * T;
  int ok = 1;
  DIRECT_PLANCHECK_UNROLL
  for (int d = 0; d < 3; d++) {
    double s[6];
    DIRECT_PLANCHECK_UNROLL
    for (int m = 0; m < 6; m++) s[m] = (double)a[m * 3 + d] * Tm[m];
    DIRECT_PLANCHECK_UNROLL
    for (int j = 0; j < 6; j++) {
      double b = 0.0;
      DIRECT_PLANCHECK_UNROLL
      for (int m = 0; m <= j; m++) {
        const double w = binom[j][m] / binom[5][m];
        const double t = w * s[m];
        b = m == 0 ? t : b + t;
      }
      P[d * 6 + j] = b;
      ok &= fabs(b) <= kMaxCoord ? 1 : 0;
    }
  }
  return ok;
}

// One de Casteljau halving of the six points of every axis, in place: right == 0 keeps the left half.  Every new point is
// (a + b) * 0.5.
DIRECT_PLANCHECK_HD void halve(double* P, int right) {
  DIRECT_PLANCHECK_NO_CONTRACT
  DIRECT_PLANCHECK_UNROLL
  for (int a = 0; a < 3; a++) {
    double w[6], L[6], R[6];
    DIRECT_PLANCHECK_UNROLL
    for (int j = 0; j < 6; j++) w[j] = P[a * 6 + j];
    L[0] = w[0];
    R[5] = w[5];
    DIRECT_PLANCHECK_UNROLL
    for (int lvl = 1; lvl < 6; lvl++) {
      DIRECT_PLANCHECK_UNROLL
      for (int j = 0; j + lvl < 6; j++) w[j] = (w[j] + w[j + 1]) * 0.5;
      L[lvl] = w[0];
      R[5 - lvl] = w[5 - lvl];
    }
    DIRECT_PLANCHECK_UNROLL
    for (int j = 0; j < 6; j++) P[a * 6 + j] = right ? R[j] : L[j];
  }
}

// The points of node (d, k) from the segment's: d halvings, step l chosen by bit d-1-l of k
DIRECT_PLANCHECK_HD void derive(const double* __restrict__ P0, int d, int k, double* __restrict__ P) {
  DIRECT_PLANCHECK_UNROLL
  for (int q = 0; q < 18; q++) P[q] = P0[q];
  for (int l = 0; l < d; l++) halve(P, (k >> (d - 1 - l)) & 1);
}

// Voxel index of q = (coord - lower) * inv along an axis of `size` voxels: -1 below the map, size above it.  The comparisons
// come before the conversion (as in mapcloud::axis_index_clamp); a NaN q (0 * inf) counts as below.
DIRECT_PLANCHECK_HD int axis_voxel(double q, int size) {
  if (q >= (double)size) return size;
  if (!(q >= 0.0)) return -1;
  return (int)q;
}

// Index box lo[3], hi[3] of the six points per axis; returns 1 when the box leaves the map
DIRECT_PLANCHECK_HD int box_of(const double* P, const Grid& G, int* lo, int* hi) {
  DIRECT_PLANCHECK_NO_CONTRACT
  int leaves = 0;
  DIRECT_PLANCHECK_UNROLL
  for (int a = 0; a < 3; a++) {
    double mn = P[a * 6], mx = P[a * 6];
    DIRECT_PLANCHECK_UNROLL
    for (int j = 1; j < 6; j++) {
      mn = P[a * 6 + j] < mn ? P[a * 6 + j] : mn;
      mx = P[a * 6 + j] > mx ? P[a * 6 + j] : mx;
    }
    const double qlo = ((mn - G.margin) - G.lower[a]) * G.inv;
    const double qhi = ((mx + G.margin) - G.lower[a]) * G.inv;
    lo[a] = axis_voxel(qlo, G.size[a]);
    hi[a] = axis_voxel(qhi, G.size[a]);
    leaves |= (lo[a] == -1 || hi[a] == G.size[a]) ? 1 : 0;
  }
  return leaves;
}

// The box's intersection with the map; 0 when it is empty
DIRECT_PLANCHECK_HD int clamp_box(const int* lo, const int* hi, const int* size, int* clo, int* chi) {
  int any = 1;
  DIRECT_PLANCHECK_UNROLL
  for (int a = 0; a < 3; a++) {
    clo[a] = lo[a] < 0 ? 0 : lo[a];
    chi[a] = hi[a] > size[a] - 1 ? size[a] - 1 : hi[a];
    any &= clo[a] <= chi[a] ? 1 : 0;
  }
  return any;
}

// Plan time at which leaf / subtree k of depth d starts: S + (k * 2^-d) * T, the factor exact, the product rounded, then the
// sum.  Its end is node_time(S, T, d, k + 1).
DIRECT_PLANCHECK_HD double node_time(double S, double T, int d, int k) {
  DIRECT_PLANCHECK_NO_CONTRACT
  const double f = (double)k * (1.0 / (double)(1 << d));
  const double p = f * T;
  return S + p;
}

// Flags of the box of points P: bit 0 occupied (occupied(lo, hi) is asked for a non-empty intersection with the map only and gets
// the clamped box), bit 1 leaves the map.  *blocked: occupied, or outside_blocks and leaving.
template <class Occupied>
DIRECT_PLANCHECK_HD int judge(const double* P, const Grid& G, Occupied&& occupied, int* lo, int* hi, int* blocked) {
  const int leaves = box_of(P, G, lo, hi);
  int clo[3], chi[3];
  const int occ = clamp_box(lo, hi, G.size, clo, chi) ? (occupied(clo, chi) ? 1 : 0) : 0;
  *blocked = occ | (G.outside_blocks ? leaves : 0);
  return occ | (leaves << 1);
}

// The first blocked judged leaf (its index at depth D) in the subtree (d0, k0) of the segment with control points P0, start S
// and duration T, or kNone; kOpen when `budget` >= 0 nodes were examined without an answer.  has_from == 0 judges every leaf.
// visit(d, k, lo, hi, flags) is told every node whose box is formed (the CPU tests check the nesting there).  No stack: the
// points of a left child come from one halving of the current ones, every other move re-derives from P0.
template <class Occupied, class Visit>
DIRECT_PLANCHECK_HD int descend(const double* __restrict__ P0, double S, double T, int D, int d0, int k0, int has_from, double t_from,
                                const Grid& G, Occupied&& occupied, Visit&& visit, int budget, long long* tests) {
  double cur[18];
  int d = d0, k = k0, seen = 0;
  derive(P0, d, k, cur);
  for (;;) {
    int blocked = 0;
    if (!has_from || node_time(S, T, d, k + 1) > t_from) {
      if (budget >= 0 && seen == budget) return kOpen;
      seen++;
      int lo[3], hi[3];
      const int flags = judge(cur, G, occupied, lo, hi, &blocked);
      visit(d, k, lo, hi, flags);
      *tests += 1;
    }
    if (blocked) {
      if (d == D) return k;
      d++;
      k <<= 1;
      halve(cur, 0);
      continue;
    }
    while (d > d0 && (k & 1)) {
      k >>= 1;
      d--;
    }
    if (d == d0) return kNone;
    k += 1;
    derive(P0, d, k, cur);
  }
}

}  // namespace plancheck
}  // namespace direct
