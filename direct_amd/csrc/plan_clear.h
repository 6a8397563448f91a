// Kernels of direct_cluster_plan_clearance_batch (include/direct_cluster.h, "metric clearance of plans"); included by
// direct_cluster.hip inside its anonymous namespace, after plan_check.h, whose PlanRows (with its helpers) and k_plan_starts serve here
// too.  The arithmetic is plan_clear_math.h's and plan_check_math.h's, shared with the CPU tests; the field is the resident one.
//
//   k_plan_starts  plan_check.h's: start times S and the row's validity into the workspace.
//   k_clear_seg    one wave per (row, segment) slot, a fixed grid striding over the slots.  Lane l owns subtree l of depth
//                  min(D, 6), as in k_plan_deep: it derives that subtree's points by its own halvings and evaluates every leaf
//                  below it - there is no pruning, every leaf contributes.  A butterfly of planclear::merge over the lanes (the
//                  minimum of the doubles, then the lowest leaf among the lanes that hold it) is the slot's minimum, its leaf and
//                  its first leaf below the radius; merge is commutative and associative, so the order of evaluation shows nowhere.
//   k_clear_rows   one wave per row, in the shape of k_plan_rows: the minimum over the segments (the first segment among equal
//                  values), the first segment with a leaf below the radius, both leaves' start times, and every row output.  A
//                  segment whose control points are not usable (kBadCoef) makes the row invalid here.
// No persistent kernel, no spin wait, no atomic of any kind; every loop is a bounded pass over leaves or a strided pass over an array.
#pragma once
#include "plan_clear_math.h"

namespace pcl = direct::planclear;

constexpr int kClearBlocks = 1024;  // workgroups of k_clear_seg (4 waves each)

struct ClearDev {
  PlanRows R;
  pcl::Grid G;
  double radius;
  const int32_t* field;             // the resident distance field
  int YZ, Z;
  double* ws_min;                   // [batch][nmax] a segment's minimum bound
  int* ws_leaf;                     // [batch][nmax] its leaf, kNoLeaf or kBadCoef
  int* ws_below;                    // [batch][nmax] its first leaf below the radius or kNoLeaf
  int32_t *status, *verdict, *where;
  double *clearance, *t_min, *t_free, *seg_clearance;
};

template <typename St>
__global__ __launch_bounds__(256) void k_clear_seg(ClearDev A) {
  const PlanRows& R = A.R;
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
  const int total = R.batch * R.nmax;
  const int dl = plan_lane_depth(R);
  const auto d2_at = [&](int i0, int i1, int i2) { return A.field[(size_t)i0 * A.YZ + (size_t)i1 * A.Z + i2]; };
  for (int g = wave; g < total; g += waves) {
    const auto [b, i] = plan_slot(R, g);
    const double* S = plan_S(R, b);
    if (!plan_row_valid(S) || i >= R.n_seg[b]) continue;  // wave-uniform
    const double Ti = (double)((const St*)R.T)[g];
    double P[18];
    if (!plan_ctrl<St>(R, g, Ti, P)) {  // wave-uniform
      if (lane == 0) A.ws_leaf[g] = pk::kBadCoef;
      continue;
    }
    pcl::SegMin r = {(double)INFINITY, pcl::kNoLeaf, pcl::kNoLeaf};
    if (lane < (1 << dl))
      r = pcl::subtree_min(P, S[i], Ti, R.depth, dl, lane, R.has_from, plan_t_from(R, b), A.radius, A.G, d2_at);
    for (int o = 32; o > 0; o >>= 1) {
      pcl::SegMin other;
      other.best = __shfl_xor(r.best, o);
      other.leaf = __shfl_xor(r.leaf, o);
      other.below = __shfl_xor(r.below, o);
      r = pcl::merge(r, other);
    }
    if (lane == 0) {
      A.ws_min[g] = r.best;
      A.ws_leaf[g] = r.leaf;
      A.ws_below[g] = r.below;
    }
  }
}

template <typename St>
__global__ __launch_bounds__(64) void k_clear_rows(ClearDev A) {
  const PlanRows& R = A.R;
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* S = plan_S(R, b);
  const int n = R.n_seg[b];
  const size_t row = (size_t)b * R.nmax;
  int valid = plan_row_valid(S) ? 1 : 0;  // wave-uniform; a valid row has 1 <= n <= nmax
  const double inf = (double)INFINITY, nan = __builtin_nan("");
  double best = inf;
  int seg = pcl::kNoLeaf, low = pcl::kNoLeaf, bad = 0;  // segment of the minimum, first segment with a leaf below the radius
  if (valid)
    for (int i = lane; i < n; i += 64) {
      const int leaf = A.ws_leaf[row + i];
      if (leaf == pk::kBadCoef) {
        bad = 1;
        continue;
      }
      const double v = A.ws_min[row + i];
      if (v < best) {
        best = v;
        seg = i;
      }
      if (A.ws_below[row + i] != pcl::kNoLeaf && low == pcl::kNoLeaf) low = i;
    }
  if (__ballot(bad)) valid = 0;
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int os = __shfl_xor(seg, o), ol = __shfl_xor(low, o);
    const double m = ob < best ? ob : best;
    const int sa = best == m ? seg : pcl::kNoLeaf, sb = ob == m ? os : pcl::kNoLeaf;
    best = m;
    seg = sb < sa ? sb : sa;
    low = ol < low ? ol : low;
  }
  if (A.seg_clearance) {
    const int cnt = n < 0 ? 0 : (n > R.nmax ? R.nmax : n);
    for (int i = lane; i < cnt; i += 64) A.seg_clearance[row + i] = valid ? A.ws_min[row + i] : nan;
  }
  if (lane != 0) return;
  int leaf = -1, s_out = -1, verdict = DIRECT_PLAN_CHECK_INVALID;
  double clearance = nan, t_min = 0.0, t_free = 0.0;
  if (valid) {
    clearance = best;
    t_min = t_free = S[n];
    verdict = 0;
    if (seg != pcl::kNoLeaf) {
      s_out = seg;
      leaf = A.ws_leaf[row + seg];
      t_min = pk::node_time(S[seg], (double)((const St*)R.T)[row + seg], R.depth, leaf);
    }
    if (low != pcl::kNoLeaf) {
      verdict = 1;
      t_free = pk::node_time(S[low], (double)((const St*)R.T)[row + low], R.depth, A.ws_below[row + low]);
    }
  }
  A.status[b] = valid ? 0 : -1;
  if (A.verdict) A.verdict[b] = verdict;
  if (A.clearance) A.clearance[b] = clearance;
  if (A.t_min) A.t_min[b] = t_min;
  if (A.t_free) A.t_free[b] = t_free;
  if (A.where) { A.where[2 * b] = s_out; A.where[2 * b + 1] = leaf; }
}

// Enqueues the three kernels for one storage type.
template <typename St>
hipError_t plan_clear_launch(const ClearDev& A, hipStream_t stream) {
  const int slots = A.R.batch * A.R.nmax;
  hipLaunchKernelGGL(k_plan_starts<St>, dim3((A.R.batch + 63) / 64), dim3(64), 0, stream, A.R);
  hipLaunchKernelGGL(k_clear_seg<St>, dim3(std::min(kClearBlocks, (slots + 3) / 4)), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(k_clear_rows<St>, dim3(A.R.batch), dim3(64), 0, stream, A);
  return hipGetLastError();
}
