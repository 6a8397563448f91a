// Kernels of direct_cluster_plan_check_batch (include/direct_cluster.h, "plans against the resident map"); included by
// direct_cluster.hip inside its anonymous namespace.  The arithmetic is plan_check_math.h's, shared with the CPU tests; the box test
// is box_obstacles() on the handle's summed-area table (eight loads), asked for the box's intersection with the map only.
//
//   PlanRows       what every kernel over plan rows reads, with the spellings that go with it: plan_clear.h's kernels use both.
//   k_plan_starts  one thread per row: the segment start times S (the evaluation's left-to-right sum) into the workspace and the
//                  row's validity as far as n_seg, T and t_from decide it (S[0] = NaN marks an invalid row, as k_eval_starts does).
//   k_plan_seg     one lane per (row, segment) slot: control points in metres, then the descent from the segment's root with a
//                  budget of kSegBudget box tests.  A free segment costs one test, a segment wholly before t_from none; most
//                  segments that are blocked at the root but clear a few levels down resolve here too.  A slot whose budget runs out
//                  goes to the list of unresolved slots: one wave ballot, one vector atomic add per wave that has any.  The order
//                  of the list shows in no output (every listed slot writes its own seg_first entry).
//   k_plan_deep    one wave per listed slot, a fixed grid striding over the list (its length never comes back to the host between the
//                  kernels).  Lane l owns subtree l of depth min(D, 6): it derives that subtree's points by its own halvings
//                  and descends it without a stack, jumping over unblocked and skipped subtrees; a wave minimum over the lanes'
//                  leaves is the segment's first.  One lane per segment instead would leave 63 lanes idle behind up to 2^13
//                  dependent table look-ups.
//   k_plan_rows    one wave per row: the first segment with a blocked leaf, in segment order, then that leaf's box, flags and
//                  start time again from the segment's coefficients, and every row output.  A segment whose control points are
//                  not usable (kBadCoef) makes the row invalid here.
// No persistent kernel, no spin wait, no floating-point atomic; every loop is a bounded tree walk or a strided pass over an array.
#pragma once
#include "plan_check_math.h"
#include "traj_eval_math.h"  // eval::row_starts

namespace pk = direct::plancheck;

constexpr int kSegBudget = 8;       // box tests a slot may spend in k_plan_seg
constexpr int kDeepBlocks = 1024;   // workgroups of k_plan_deep (4 waves each)

// The caller's rows and the start times k_plan_starts leaves in the call's workspace; slot g is segment g % nmax of row g / nmax.
struct PlanRows {
  int batch, nmax, depth, poly, has_from;
  const int32_t* n_seg;
  const void *T, *coef;             // the storage type's
  const double* t_from;
  double* S;                        // [batch][nmax + 1]
};

template <typename St>  // control points in metres of slot g, whose duration is Ti; 0 when they are not usable
__device__ __forceinline__ int plan_ctrl(const PlanRows& R, int g, double Ti, double* P) {
  const St* c = (const St*)R.coef + (size_t)g * 18;
  return R.poly ? pk::ctrl_from_poly(c, Ti, P) : pk::ctrl_from_bez(c, Ti, P);
}
struct PlanSlot { int b, i; };  // row and segment
__device__ __forceinline__ PlanSlot plan_slot(const PlanRows& R, int g) { return {g / R.nmax, g - g / R.nmax * R.nmax}; }
__device__ __forceinline__ double* plan_S(const PlanRows& R, int b) { return R.S + (size_t)b * (R.nmax + 1); }
__device__ __forceinline__ bool plan_row_valid(const double* S) { return S[0] == 0.0; }  // k_plan_starts left no NaN there
__device__ __forceinline__ double plan_t_from(const PlanRows& R, int b) { return R.has_from ? R.t_from[b] : 0.0; }
__device__ __forceinline__ int plan_lane_depth(const PlanRows& R) { return R.depth < 6 ? R.depth : 6; }

struct PlanDev {
  pk::Grid G;                       // first: the row fields then sit where the kernels' arguments always had them
  PlanRows R;
  int count;
  int* ws_first;                    // [batch][nmax] a segment's first blocked judged leaf, kNone or kBadCoef
  int* list;                        // [batch * nmax] unresolved slots
  unsigned* n_list;                 // [1]
  unsigned long long* n_tests;      // [1] box tests, counted when `count` is set
  int32_t *status, *verdict, *first, *hit_box, *seg_first;
  double* t_free;
};

__device__ __forceinline__ void plan_count(const PlanDev& A, long long tests) {
  if (!A.count) return;
  for (int o = 32; o > 0; o >>= 1) tests += __shfl_down(tests, o);
  if ((threadIdx.x & 63) == 0 && tests) atomicAdd(A.n_tests, (unsigned long long)tests);
}

template <typename St>
__global__ __launch_bounds__(64) void k_plan_starts(PlanRows R) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= R.batch) return;
  double* S = plan_S(R, b);
  int ok = direct::eval::row_starts((const St*)R.T + (size_t)b * R.nmax, R.n_seg[b], R.nmax, S);
  if (R.has_from && R.t_from[b] != R.t_from[b]) ok = 0;
  if (!ok) S[0] = __builtin_nan("");
}

template <typename St>
__global__ __launch_bounds__(256) void k_plan_seg(Dev D, PlanDev A) {
  const PlanRows& R = A.R;
  const int g = blockIdx.x * 256 + threadIdx.x, total = R.batch * R.nmax;
  const auto occupied = [&](const int* lo, const int* hi) { return box_obstacles(D, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]) > 0; };
  const auto visit = [](int, int, const int*, const int*, int) {};
  long long tests = 0;
  int open = 0;
  if (g < total) {
    const auto [b, i] = plan_slot(R, g);
    const double* S = plan_S(R, b);
    if (plan_row_valid(S) && i < R.n_seg[b]) {
      const double Ti = (double)((const St*)R.T)[g];
      double P[18];
      int r = pk::kBadCoef;
      if (plan_ctrl<St>(R, g, Ti, P))
        r = pk::descend(P, S[i], Ti, R.depth, 0, 0, R.has_from, plan_t_from(R, b), A.G, occupied, visit, kSegBudget, &tests);
      if (r == pk::kOpen) open = 1;
      else A.ws_first[g] = r;
    }
  }
  const unsigned long long m = __ballot(open);
  if (m) {
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(A.n_list, (unsigned)__popcll(m));
    base = __shfl(base, leader);
    if (open) A.list[base + __popcll(m & ((1ull << lane) - 1ull))] = g;
  }
  plan_count(A, tests);
}

template <typename St>
__global__ __launch_bounds__(256) void k_plan_deep(Dev D, PlanDev A) {
  const PlanRows& R = A.R;
  const auto occupied = [&](const int* lo, const int* hi) { return box_obstacles(D, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]) > 0; };
  const auto visit = [](int, int, const int*, const int*, int) {};
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
  const unsigned n = *A.n_list;  // final: k_plan_seg has ended
  const int dl = plan_lane_depth(R);
  long long tests = 0;
  for (unsigned idx = wave; idx < n; idx += waves) {
    const int g = A.list[idx];
    const auto [b, i] = plan_slot(R, g);
    const double Ti = (double)((const St*)R.T)[g];
    double P[18];
    (void)plan_ctrl<St>(R, g, Ti, P);  // usable: the slot was listed
    int r = pk::kNone;
    if (lane < (1 << dl))
      r = pk::descend(P, plan_S(R, b)[i], Ti, R.depth, dl, lane, R.has_from, plan_t_from(R, b), A.G, occupied, visit, -1, &tests);
    int key = r >= 0 ? r : 0x7fffffff;
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(key, o);
      key = other < key ? other : key;
    }
    if (lane == 0) A.ws_first[g] = key == 0x7fffffff ? pk::kNone : key;
  }
  plan_count(A, tests);
}

template <typename St>
__global__ __launch_bounds__(64) void k_plan_rows(Dev D, PlanDev A) {
  const PlanRows& R = A.R;
  const auto occupied = [&](const int* lo, const int* hi) { return box_obstacles(D, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]) > 0; };
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* S = plan_S(R, b);
  const int n = R.n_seg[b];
  const int* ws = A.ws_first + (size_t)b * R.nmax;
  int valid = plan_row_valid(S) ? 1 : 0;  // wave-uniform
  int best = 0x7fffffff, bad = 0;
  if (valid)
    for (int i = lane; i < n; i += 64) {
      const int v = ws[i];
      bad |= v == pk::kBadCoef ? 1 : 0;
      if (v >= 0 && best == 0x7fffffff) best = i;
    }
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(best, o);
    best = other < best ? other : best;
  }
  if (__ballot(bad)) valid = 0;
  if (A.seg_first) {
    const int cnt = n < 0 ? 0 : (n > R.nmax ? R.nmax : n);
    for (int i = lane; i < cnt; i += 64) A.seg_first[(size_t)b * R.nmax + i] = valid ? ws[i] : -1;
  }
  int verdict = valid ? 0 : -1, seg = -1, leaf = -1, box[6] = {-1, -1, -1, -1, -1, -1};
  double t_free = valid ? S[n] : 0.0;
  if (valid && best != 0x7fffffff) {
    const int g = b * R.nmax + best;
    const double Ti = (double)((const St*)R.T)[g];
    double P[18], L[18];
    (void)plan_ctrl<St>(R, g, Ti, P);
    seg = best;
    leaf = ws[best];
    pk::derive(P, R.depth, leaf, L);
    int blocked;
    verdict = pk::judge(L, A.G, occupied, box, box + 3, &blocked);
    t_free = pk::node_time(S[best], Ti, R.depth, leaf);
  }
  if (lane == 0) {
    A.status[b] = valid ? 0 : -1;
    if (A.verdict) A.verdict[b] = verdict;
    if (A.t_free) A.t_free[b] = t_free;
    if (A.first) { A.first[2 * b] = seg; A.first[2 * b + 1] = leaf; }
    if (A.hit_box)
      for (int q = 0; q < 6; q++) A.hit_box[6 * (size_t)b + q] = box[q];
  }
}

// Enqueues the four kernels for one storage type; the counters of the workspace have been cleared on the same stream.
template <typename St>
hipError_t plan_check_launch(const Dev& D, const PlanDev& A, hipStream_t stream) {
  const int slots = A.R.batch * A.R.nmax;
  hipLaunchKernelGGL(k_plan_starts<St>, dim3((A.R.batch + 63) / 64), dim3(64), 0, stream, A.R);
  hipLaunchKernelGGL(k_plan_seg<St>, dim3((slots + 255) / 256), dim3(256), 0, stream, D, A);
  if (A.R.depth > 0)  // at depth 0 the root is the leaf: nothing can stay open
    hipLaunchKernelGGL(k_plan_deep<St>, dim3(std::min(kDeepBlocks, (slots + 3) / 4)), dim3(256), 0, stream, D, A);
  hipLaunchKernelGGL(k_plan_rows<St>, dim3(A.R.batch), dim3(64), 0, stream, D, A);
  return hipGetLastError();
}
