// Arithmetic of direct_cluster_plan_clearance_batch (include/direct_cluster.h, "metric clearance of plans"): the lower bound of one
// leaf's distance to the occupied voxels from the resident distance field, the minimum over a subtree of leaves, and the merge of two
// such minima.  Rows, control points, halvings and leaf times are plan_check_math.h's and are not restated here.  Plain C++ behind a
// qualifier macro: the kernels of plan_clear.h call these functions, and g++ compiles the same header for the CPU tests
// (tests/dist_field_harness.py).
//
// Everything is double, written with plain *, +, - and sqrt and no fma(), and contraction is off (the pragma below under clang; g++
// gets -ffp-contract=off from the harness): the NumPy restatement performs the same operations and must get the same bits.
//
// Why leaf_bound() is a lower bound.  Let m be the centre of the voxel the box centre c is clamped into and d2 the field there.
// The nearest occupied voxel CENTRE is resolution * sqrt(d2) from m, and an occupied cube reaches at most sqrt(3)/2 * resolution
// from its centre, so the occupied set is at least (sqrt(d2) - sqrt(3)/2) * resolution from m.  The distance to a set is
// 1-Lipschitz and c is `off` from m, so the set is at least that minus `off` from c.  Every point of the leaf's piece of curve lies
// in the box of its control points (convex hull), hence within `half` of c: the piece is at least that minus `half` from the set.
// A box centre outside the map goes through the same formula with the clamped voxel, `off` carrying the displacement.  A capped
// field only lowers d2, so the bound stays valid.  kK is the smallest double not below sqrt(3)/2, so rounding it does not weaken
// the bound.  NOT an exact predicate: certified up to the rounding of the fifteen-odd double operations below, about 1e-15
// relative.  A negative bound is reported as computed and means "nothing certified".
#pragma once
#include <math.h>
#include <stdint.h>

#include "plan_check_math.h"

namespace direct {
namespace planclear {

namespace pk = direct::plancheck;

constexpr double kK = 0x1.bb67ae8584cabp-1;  // 0.8660254037844387: sqrt(3)/2 rounded up (the double below is 5e-17 short of it)
constexpr int kDistNone = 0x7fffffff;        // DIRECT_DIST_NONE
constexpr int kNoLeaf = 0x7fffffff;          // no such leaf

struct Grid {
  double lower[3];
  double inv, resolution;
  int size[3];
};

// The voxel index q = (coord - lower) * inv is clamped into, compared before it is converted (mapcloud::axis_index_clamp's rule);
// a NaN q counts as below.
DIRECT_PLANCHECK_HD int axis_cell(double q, int size) {
  if (q >= (double)size) return size - 1;
  if (!(q >= 1.0)) return 0;
  return (int)q;
}

// The bound of the leaf with points L[a * 6 + j]; d2_at(i0, i1, i2) reads the stored field.  *half_out: the box's half-diagonal.
template <class Field>
DIRECT_PLANCHECK_HD double leaf_bound(const double* L, const Grid& G, Field&& d2_at, double* half_out) {
  DIRECT_PLANCHECK_NO_CONTRACT
  double e[3], r[3];
  int idx[3];
  DIRECT_PLANCHECK_UNROLL
  for (int a = 0; a < 3; a++) {
    double lo = L[a * 6], hi = L[a * 6];
    DIRECT_PLANCHECK_UNROLL
    for (int j = 1; j < 6; j++) {
      lo = L[a * 6 + j] < lo ? L[a * 6 + j] : lo;
      hi = L[a * 6 + j] > hi ? L[a * 6 + j] : hi;
    }
    const double c = (lo + hi) * 0.5;
    e[a] = (hi - lo) * 0.5;
    const double q = (c - G.lower[a]) * G.inv;
    idx[a] = axis_cell(q, G.size[a]);
    const double m = ((double)idx[a] + 0.5) * G.resolution + G.lower[a];
    r[a] = c - m;
  }
  const double half = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
  const double off = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
  *half_out = half;
  const int d2 = d2_at(idx[0], idx[1], idx[2]);
  if (d2 == kDistNone) return (double)INFINITY;
  return ((sqrt((double)d2) - kK) * G.resolution - off) - half;
}

// Minimum of the judged leaves of a set: the bound, its first leaf in leaf order (kNoLeaf while the bound is +inf), and the first
// judged leaf whose bound is below the radius (kNoLeaf: none)
struct SegMin {
  double best;
  int leaf, below;
};

// Of two disjoint sets of leaves.  Commutative and associative, so the result does not depend on the order of evaluation.
DIRECT_PLANCHECK_HD SegMin merge(const SegMin& a, const SegMin& b) {
  SegMin r;
  r.best = b.best < a.best ? b.best : a.best;
  const int la = a.best == r.best ? a.leaf : kNoLeaf, lb = b.best == r.best ? b.leaf : kNoLeaf;
  r.leaf = lb < la ? lb : la;
  r.below = b.below < a.below ? b.below : a.below;
  return r;
}

// The leaves of depth D below node (d0, k0) of the segment with control points P0, start S and duration T, every one visited.
// has_from == 0 judges every leaf; otherwise a leaf is judged iff its end time is > t_from.
template <class Field>
DIRECT_PLANCHECK_HD SegMin subtree_min(const double* __restrict__ P0, double S, double T, int D, int d0, int k0, int has_from,
                                       double t_from, double radius, const Grid& G, Field&& d2_at) {
  double sub[18], L[18];
  pk::derive(P0, d0, k0, sub);
  const int m = D - d0;
  SegMin r = {(double)INFINITY, kNoLeaf, kNoLeaf};
  for (int kk = 0; kk < (1 << m); kk++) {
    const int k = (k0 << m) + kk;
    if (has_from && !(pk::node_time(S, T, D, k + 1) > t_from)) continue;
    pk::derive(sub, m, kk, L);
    double half;
    const double b = leaf_bound(L, G, d2_at, &half);
    if (b < r.best) {
      r.best = b;
      r.leaf = k;
    }
    if (b < radius && r.below == kNoLeaf) r.below = k;
  }
  return r;
}

}  // namespace planclear
}  // namespace direct
