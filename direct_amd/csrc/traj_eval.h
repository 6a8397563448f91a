// Trajectory evaluation at caller-given times (include/direct_ddp.h, direct_traj_eval_batch): position .. snap, the segment
// and the [p, v, a] state of a solved plan on ONE clock - seconds from the trajectory's start - for every query of a batch.
// No reference counterpart: the reference's consumers (PositionCommand set-points, replanning from the current state) need
// exactly these values, its own sampler (traj_sample.h) restarts time in every segment.
//
// Two kernels.  k_eval_starts (one thread per trajectory) sums the durations left to right into the segment start times
// S[b][0..n] of a workspace, judges the row (status) and writes t_total: the sequential sum is done ONCE per row, not once
// per wave (0.03 ms per call at B = 32768, N = 100; the same sum by one lane of every k_eval wave instead made k_eval 0.11 ms
// slower).  k_eval: grid (query chunks, batch), one 64-lane wave per chunk of kEvalChunk consecutive queries, lane l of
// the chunk handling queries q0 + l + 64 k.  A wave
//   1. copies S of its row into LDS and finds every query's segment by a halving search (traj_eval_math.h, locate);
//   2. stages the tables of the segments its chunk spans (at most kEvalSlots: differences of the control points or the
//      monomial coefficients, in double) into LDS, one segment per lane;
//   3. evaluates and stores.
// Every load of the wave is issued before its first store: vector loads share the in-order vmcnt counter with the stores,
// so a load between stores would wait for every earlier store to drain (the lesson of k_sample).  A chunk
// that spans more segments than the slots (explicit times in no particular order) falls back to per-query loads of the
// segment's coefficients from global memory (any grid of fewer than ~8 queries per segment: bench case "coarse").
// Not bound by its stores: the same stores with nothing loaded or computed run at 5.8 TB/s, the kernel at 3.4 TB/s; the
// difference is each wave's loads, search and arithmetic ahead of its stores, which 5 waves per SIMD do not hide.
#pragma once
#include <hip/hip_runtime.h>

#include "traj_eval_math.h"
#include "traj_sample.h"  // store3

namespace direct {

constexpr int kEvalQ = 4;                // queries per lane and chunk (2 and 8 measured no faster)
constexpr int kEvalChunk = 64 * kEvalQ;  // consecutive queries per wave
constexpr int kEvalSlots = 32;           // segments a chunk may span and still have their tables staged in LDS
constexpr int kEvalSCap = 1024;          // rows of fewer segments search S in LDS, longer ones in the workspace (global memory)

template <typename St>
struct EvalArgs {
  int batch, nmax, m_max, poly, b_off;
  const int32_t* n_seg;
  const St* T;
  const St* coef;  // bez or poly, [batch][nmax][18]
  const int32_t* n_query;
  const St* t;
  double t0, dt;
  double* S;  // workspace [batch][nmax + 1]; S[b][0] = NaN marks an invalid row
  int32_t* status;
  St* t_total;
  int32_t* seg;
  St* out[5];  // pos, vel, acc, jerk, snap
  St* state;
};

// lds bytes of one k_eval wave for rows of up to nmax segments
__host__ __device__ inline size_t eval_lds_bytes(int nmax) {
  return (size_t)(kEvalSlots * eval::kTab + (nmax < kEvalSCap ? nmax : kEvalSCap - 1) + 1) * sizeof(double);
}

template <typename St>
__global__ __launch_bounds__(64) void k_eval_starts(EvalArgs<St> A) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= A.batch) return;
  double* S = A.S + (size_t)b * (A.nmax + 1);
  const int n = A.n_seg[b];
  const int ok = eval::row_starts(A.T + (size_t)b * A.nmax, n, A.nmax, S);
  if (!ok) S[0] = __builtin_nan("");
  A.status[b] = ok ? 0 : -1;
  if (A.t_total) A.t_total[b] = (St)(ok ? S[n] : 0.0);
}

// seg and the requested outputs of query i (o[k * 3 + d], k = 0..4)
template <typename St>
__device__ __forceinline__ void eval_put(const EvalArgs<St>& A, size_t i, int seg, const double* o) {
  if (A.seg) A.seg[i] = seg;
#pragma unroll
  for (int k = 0; k < 5; k++)
    if (A.out[k]) store3(A.out[k] + i * 3, o[3 * k], o[3 * k + 1], o[3 * k + 2]);
  if (A.state) {
    store3(A.state + i * 9, o[0], o[1], o[2]);
    store3(A.state + i * 9 + 3, o[3], o[4], o[5]);
    store3(A.state + i * 9 + 6, o[6], o[7], o[8]);
  }
}

// the table of segment i of row b, straight from global memory
template <bool kPoly, typename St>
__device__ __forceinline__ void eval_load_table(const EvalArgs<St>& A, int b, int i, double* tab) {
  const St* c = A.coef + ((size_t)b * A.nmax + i) * 18;
  double raw[18];
#pragma unroll
  for (int q = 0; q < 18; q++) raw[q] = (double)c[q];
  if (kPoly)
    eval::poly_table(raw, tab);
  else
    eval::bez_table(raw, (double)A.T[(size_t)b * A.nmax + i], tab);
}

template <bool kPoly>
__device__ __forceinline__ void eval_point(const double* tab, double s, double* o) {
  if (kPoly)
    eval::eval_poly(tab, s, o);
  else
    eval::eval_bez(tab, eval::bez_tau(s, tab), o);
}

// steps 1-3 of the header for one chunk, S in LDS or in the workspace.  The source (bez / poly) is a template argument: with
// a run-time choice the compiler merged the two table layouts of the fallback path into one private array (scratch).
template <bool kPoly, typename St>
__device__ __forceinline__ void eval_chunk(const EvalArgs<St>& A, int b, int n, int q0, int nq, const double* S, double* tabs) {
  const int lane = threadIdx.x;
  const size_t ob = (size_t)b * A.m_max;
  int sg[kEvalQ];
  double sl[kEvalQ];
  int lo = 0x7fffffff, hi = -1;
#pragma unroll
  for (int k = 0; k < kEvalQ; k++) {
    const int q = q0 + k * 64 + lane;
    double t = 0.0;
    if (q < nq) t = A.t ? (double)A.t[ob + q] : eval::grid_time(A.t0, q, A.dt);
    const eval::Loc L = eval::locate(S, n, t);
    sl[k] = L.s;
    sg[k] = q < nq ? L.seg : -2;  // -2: past n_query, nothing is written
    if (sg[k] >= 0) {
      lo = min(lo, L.seg);
      hi = max(hi, L.seg);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  const bool staged = hi < lo || hi - lo < kEvalSlots;  // hi < lo: no query of the chunk has a segment
  if (staged) {
    if (hi >= lo && lane <= hi - lo) eval_load_table<kPoly>(A, b, lo + lane, tabs + lane * eval::kTab);
    __syncthreads();
  }
  const double nan = __builtin_nan("");
#pragma unroll
  for (int k = 0; k < kEvalQ; k++) {
    if (sg[k] == -2) continue;
    double o[15];
    if (sg[k] < 0) {
#pragma unroll
      for (int j = 0; j < 15; j++) o[j] = nan;
    } else if (staged) {
      eval_point<kPoly>(tabs + (sg[k] - lo) * eval::kTab, sl[k], o);
    } else {
      double tab[eval::kTab];
      eval_load_table<kPoly>(A, b, sg[k], tab);
      eval_point<kPoly>(tab, sl[k], o);
    }
    eval_put(A, ob + q0 + k * 64 + lane, sg[k], o);
  }
}

template <typename St>
__global__ __launch_bounds__(64) void k_eval(EvalArgs<St> A) {
  extern __shared__ __attribute__((aligned(16))) double eval_lds[];  // [kEvalSlots][kTab] segment tables, then S[0..n]
  const int lane = threadIdx.x, b = blockIdx.y + A.b_off;
  const int q0 = blockIdx.x * kEvalChunk;
  const int nq = A.n_query ? min(max(A.n_query[b], 0), A.m_max) : A.m_max;
  if (q0 >= nq) return;
  const double* Sg = A.S + (size_t)b * (A.nmax + 1);
  if (!(Sg[0] == 0.0)) {  // invalid row (k_eval_starts): seg = -1 and zeros in its first n_query entries
    const double z[15] = {};
#pragma unroll
    for (int k = 0; k < kEvalQ; k++) {
      const int q = q0 + k * 64 + lane;
      if (q < nq) eval_put(A, (size_t)b * A.m_max + q, -1, z);
    }
    return;
  }
  const int n = A.n_seg[b];  // in [1, nmax]: the row is valid
  double* tabs = eval_lds;
  if (n < kEvalSCap) {
    double* Sl = eval_lds + kEvalSlots * eval::kTab;
    for (int i = lane; i <= n; i += 64) Sl[i] = Sg[i];
    __syncthreads();
    if (A.poly)
      eval_chunk<true>(A, b, n, q0, nq, Sl, tabs);
    else
      eval_chunk<false>(A, b, n, q0, nq, Sl, tabs);
  } else if (A.poly) {
    eval_chunk<true>(A, b, n, q0, nq, Sg, tabs);
  } else {
    eval_chunk<false>(A, b, n, q0, nq, Sg, tabs);
  }
}

}  // namespace direct
