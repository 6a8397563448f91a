// Continuous-time audit of solved plans (include/direct_ddp.h, direct_traj_audit_batch): the true maxima over closed
// segments of velocity, acceleration and jerk (per axis and Euclidean), the corridor clearance of the whole curve, where
// the peaks occur on the plan's clock, the jumps across segment boundaries, a verdict word per plan and the cheapest plan
// that passes.  No reference counterpart: the reference (and traj_sample.h after it) only looks at samples.  The arithmetic
// is traj_audit_math.h, shared with the CPU tests; this file is the mapping onto the machine.
//
// Four kernels on the handle's stream.
//   k_audit_starts  one thread per row: segment start times S[b][0..n] into the workspace (S[b][0] = NaN: the row's n or
//                   durations are invalid), as k_eval_starts does.
//   k_audit_items   one 64-lane wave per 64 consecutive (row, segment) slots.  Lane l stages slot g0 + l as a record of
//                   doubles in LDS (monomial coefficients in the segment's own variable, derivative scales, S_i) and works
//                   the segment's axis items (3 axes x velocity, acceleration, jerk: ladders of depth 3, 2, 1), its norm
//                   items when asked (depth 7, 5, 3) and the jumps against the record of the lane before.  All lanes of
//                   the wave run the same ladder depth at the same time: the passes are separate loops, not one loop with
//                   a per-lane degree.  The PLANE items (depth 4) are then dealt out afresh: an exclusive scan of the 64
//                   plane counts numbers the wave's items, lane l takes items l, l + 64, ... and finds its segment in the
//                   scan by a fixed 6-step search, so a segment with 6 planes next to one with 12 idles no lane.  A round's
//                   64 (value, time) results go through LDS to the segment's own lane, which folds them in ascending plane
//                   order.  The wave writes one 16-double record per segment to the workspace.
//   k_audit_rows    one wave per row: the segments' records reduced with the contract's total order (larger value, earlier
//                   time, earlier segment, smaller plane) by butterfly shuffles - every lane ends with the same result
//                   whatever the order -, then verdict, slowdown and the outputs; the verdict also goes to the workspace.
//   k_audit_best    one workgroup: the cheapest row among verdict == 0 (and rtn >= 0), ties to the smaller index.
// No atomics and nothing that depends on arrival order: a row's outputs are a function of the row alone.
#pragma once
#include <hip/hip_runtime.h>

#include "traj_audit_math.h"

namespace direct {

constexpr int kAuditSeg = 64;  // (row, segment) slots per wave

template <typename St>
struct AuditArgs {
  int batch, nmax, pmax, poly, norms, has_planes;
  audit::Limits lim;
  const int32_t* n_seg;
  const St* T;
  const St* coef;  // bez or poly, [batch][nmax][18]
  const int32_t* n_planes;
  const St* planes;
  const St* cost;
  const int32_t* rtn;
  double* S;     // workspace [batch][nmax + 1]
  double* W;     // workspace [batch * nmax][audit::kWs]
  int32_t* V;    // workspace [batch]: verdicts
  int32_t* status;
  St* t_total;
  St* peak[7];   // vpeak, apeak, jpeak, vnorm, anorm, jnorm, cpeak
  int32_t* c_where;
  St* at;
  St* seg_peak;
  St* gap;
  int32_t* verdict;
  St* slowdown;
  long long* best;
};

// bytes of the workspace for a call of this size: S, W, V
inline size_t audit_ws_bytes(size_t batch, size_t nmax) {
  return (batch * (nmax + 1) + batch * nmax * audit::kWs) * sizeof(double) + batch * sizeof(int32_t);
}

template <typename St>
__global__ __launch_bounds__(64) void k_audit_starts(AuditArgs<St> A) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= A.batch) return;
  double* S = A.S + (size_t)b * (A.nmax + 1);
  const int ok = eval::row_starts(A.T + (size_t)b * A.nmax, A.n_seg[b], A.nmax, S);
  if (!ok) S[0] = __builtin_nan("");
}

// slot g's record into rec (LDS); returns 1 when one of its 18 coefficients is not finite
template <bool kPoly, typename St>
__device__ __forceinline__ int audit_stage(const AuditArgs<St>& A, long long g, double S, double* rec) {
  const St* c = A.coef + (size_t)g * 18;
  double raw[18], r[audit::kRec];
  int bad = 0;
#pragma unroll
  for (int q = 0; q < 18; q++) {
    raw[q] = (double)c[q];
    bad |= !audit::is_finite(raw[q]);
  }
  const double T = (double)A.T[g];
  if (kPoly)
    audit::seg_from_poly(raw, T, S, r);
  else
    audit::seg_from_bez(raw, T, S, r);
#pragma unroll
  for (int q = 0; q < audit::kRec; q++) rec[q] = r[q];
  return bad;
}

template <bool kPoly, typename St>
__global__ __launch_bounds__(64) void k_audit_items(AuditArgs<St> A) {
  __shared__ double recs[(kAuditSeg + 1) * audit::kRec];  // slot 0: the segment before the wave's first
  __shared__ int pre[kAuditSeg + 1];
  __shared__ double pv[64], pt[64];
  const int lane = threadIdx.x;
  const long long total = (long long)A.batch * A.nmax;
  const long long g0 = (long long)blockIdx.x * kAuditSeg, g = g0 + lane;
  int b = 0, i = 0;
  bool active = false;
  if (g < total) {
    b = (int)(g / A.nmax);
    i = (int)(g - (long long)b * A.nmax);
    const double* S = A.S + (size_t)b * (A.nmax + 1);
    active = S[0] == 0.0 && i < A.n_seg[b];  // a valid row has n_seg in [1, nmax]
  }
  int bad = 0;
  double* rec = recs + (lane + 1) * audit::kRec;
  if (active) {
    const double* S = A.S + (size_t)b * (A.nmax + 1);
    bad = audit_stage<kPoly>(A, g, S[i], rec);
    if (lane == 0 && i > 0) (void)audit_stage<kPoly>(A, g - 1, S[i - 1], recs);  // same row: i - 1 >= 0
  }
  __syncthreads();
  double w[audit::kWs];
  if (active) audit::segment_items(rec, i > 0 ? rec - audit::kRec : nullptr, A.norms, w);
  if (A.has_planes) {  // wave-uniform
    int np = 0;
    if (active) {
      np = A.n_planes[g];
      if (np < 1 || np > A.pmax) {
        np = 0;
        bad = 1;
      }
    }
    int incl = np;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 0) pre[0] = 0;
    pre[lane + 1] = incl;
    __syncthreads();
    const int n_items = pre[kAuditSeg];
    const int first = incl - np;
    for (int base = 0; base < n_items; base += 64) {
      const int item = base + lane;
      double v = 0.0, t = 0.0;
      if (item < n_items) {
        int s = 0;  // the largest s with pre[s] <= item
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) s = (pre[s + step] <= item) ? s + step : s;
        const int k = item - pre[s];
        const St* p = A.planes + ((size_t)(g0 + s) * A.pmax + k) * 4;
        const double pa = (double)p[0], pb = (double)p[1], pc = (double)p[2], pd = (double)p[3];
        audit::plane_peak(recs + (s + 1) * audit::kRec, pa, pb, pc, pd, v, t);
        if (!(audit::is_finite(pa) && audit::is_finite(pb) && audit::is_finite(pc) && audit::is_finite(pd))) t = __builtin_nan("");
      }
      pv[lane] = v;
      pt[lane] = t;
      __syncthreads();
      const int lo = max(first, base), hi = min(first + np, base + 64);
      for (int q = lo; q < hi; q++) {  // this segment's planes of the round, in ascending order
        const double tq = pt[q - base];
        if (tq != tq)
          bad = 1;
        else
          audit::segment_plane(w, q - first, pv[q - base], tq);
      }
      __syncthreads();
    }
  }
  if (active) {
    w[audit::W_BAD] = bad ? 1.0 : 0.0;
    double* o = A.W + (size_t)g * audit::kWs;
#pragma unroll
    for (int q = 0; q < audit::kWs; q++) o[q] = w[q];
  }
}

__device__ __forceinline__ double audit_xor(double v, int o) { return __shfl_xor(v, o, 64); }

template <typename St>
__global__ __launch_bounds__(64) void k_audit_rows(AuditArgs<St> A) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* S = A.S + (size_t)b * (A.nmax + 1);
  const int n_raw = A.n_seg[b];
  const int n = min(max(n_raw, 0), A.nmax);
  bool ok = S[0] == 0.0;
  audit::RowAcc R;
  audit::row_init(R);
  if (ok) {
    for (int i = lane; i < n; i += 64) audit::row_add(R, i, A.W + ((size_t)b * A.nmax + i) * audit::kWs, A.has_planes);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      audit::RowAcc B;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        B.v[k] = audit_xor(R.v[k], o);
        B.t[k] = audit_xor(R.t[k], o);
        B.nrm[k] = audit_xor(R.nrm[k], o);
        B.gap[k] = audit_xor(R.gap[k], o);
      }
      B.c = audit_xor(R.c, o);
      B.tc = audit_xor(R.tc, o);
      B.cseg = audit_xor(R.cseg, o);
      B.cpl = audit_xor(R.cpl, o);
      B.bad = __shfl_xor(R.bad, o, 64);
      audit::row_merge(R, B);
    }
    ok = !R.bad;
  }
  if (A.seg_peak) {  // the first n entries: the segment's four per-axis quantities, zeros on an invalid row
    for (int i = lane; i < n; i += 64) {
      const double* w = A.W + ((size_t)b * A.nmax + i) * audit::kWs;
      St* o = A.seg_peak + ((size_t)b * A.nmax + i) * 4;
#pragma unroll
      for (int q = 0; q < 4; q++) o[q] = ok ? (St)((q < 3 || A.has_planes) ? w[q] : 0.0) : (St)0;
    }
  }
  if (lane != 0) return;
  audit::RowOut O;
  if (ok) {
    audit::row_finish(R, A.lim, O);
  } else {
#pragma unroll
    for (int q = 0; q < 7; q++) O.peak[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; q++) O.at[q] = 0.0;
    O.gap[0] = O.gap[1] = O.gap[2] = O.slowdown = 0.0;
    O.c_where[0] = O.c_where[1] = 0;
    O.verdict = DIRECT_AUDIT_INVALID;
  }
  A.V[b] = O.verdict;
  A.status[b] = ok ? 0 : -1;
  if (A.t_total) A.t_total[b] = (St)(ok ? S[n] : 0.0);
#pragma unroll
  for (int q = 0; q < 7; q++)
    if (A.peak[q]) A.peak[q][b] = (St)O.peak[q];
  if (A.c_where) {
    A.c_where[2 * b] = O.c_where[0];
    A.c_where[2 * b + 1] = O.c_where[1];
  }
  if (A.at) {
#pragma unroll
    for (int q = 0; q < 4; q++) A.at[4 * (size_t)b + q] = (St)O.at[q];
  }
  if (A.gap) {
#pragma unroll
    for (int q = 0; q < 3; q++) A.gap[3 * (size_t)b + q] = (St)O.gap[q];
  }
  if (A.verdict) A.verdict[b] = O.verdict;
  if (A.slowdown) A.slowdown[b] = (St)O.slowdown;
}

template <typename St>
__global__ __launch_bounds__(256) void k_audit_best(AuditArgs<St> A) {
  __shared__ double sc[256];
  __shared__ int si[256];
  const int tid = threadIdx.x;
  double bc = 0.0;
  int bi = -1;
  for (int b = tid; b < A.batch; b += 256) {  // ascending b: a strict comparison keeps the smaller index
    const double c = (double)A.cost[b];
    if (A.V[b] == 0 && (!A.rtn || A.rtn[b] >= 0) && c == c && (bi < 0 || c < bc)) {
      bc = c;
      bi = b;
    }
  }
  sc[tid] = bc;
  si[tid] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const double c = sc[tid + o];
      const int j = si[tid + o];
      if (j >= 0 && (si[tid] < 0 || c < sc[tid] || (c == sc[tid] && j < si[tid]))) {
        sc[tid] = c;
        si[tid] = j;
      }
    }
    __syncthreads();
  }
  if (tid == 0) A.best[0] = si[0];
}

}  // namespace direct
