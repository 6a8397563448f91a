// Kernels of direct_cluster_corridor_batch (include/direct_cluster.h, "cluster corridors"): the corridors of a batch of grid paths
// in the reference's is_cluster_on == true mode, the walk on the device.  Included from direct_cluster.hip inside its anonymous
// namespace, after Dev / Elem; the rules are cluster_corridor_math.h (plain C++, also compiled by g++ for
// tests/cluster_corridor_harness.py).  The host runs ROUNDS (direct_cluster.hip):
//
//   k_corr_advance  one wave per row: the row walks until a point needs a polytope or the path ends
//   k_corr_unique   one workgroup: the due seeds of the round, de-duplicated by voxel, compacted in row order into the seed list
//   (the host reads the unique count back, then per chunk of at most max_batch seeds: generation + hull on the device seed list)
//   k_corr_append   one wave per row: a due row whose slot lies in the chunk takes its polytope onto its plane stack, or a code
//   k_corr_emit     after the last round: the stacks become the outputs, in the call's plane_dtype, zeros behind
//
// No kernel waits for another workgroup; every loop is bounded by path_len, batch, p_max or seg_capacity.  A row's walk reads only
// its own state and stack, a polytope depends on its seed voxel and the map alone, and the owner of a voxel is the smallest row:
// no output depends on the launch shape, on max_batch or on the order of the rows.
#pragma once

namespace kc = ::direct::clucor;

struct CorrDev {
  int batch, path_cap, seg_cap, p_max, pop_back;
  int X, Y, Z;
  double res, lower[3];
  const int32_t* path_xyz;  // [batch][path_cap][3]
  const int32_t* path_len;  // [batch]
  kc::Row* rows;            // [batch] the walk states
  double* st_planes;        // [batch][seg_cap][p_max][4] the plane stacks, ALWAYS double: the walk's tests read these
  int32_t* st_np;           // [batch][seg_cap]
  double *st_seeds, *st_centers;  // [batch][seg_cap][3]
  int* table;               // [X*Y*Z] owner row of a due voxel, kc::kNoOwner between rounds
  int32_t* seed_list;       // [batch][3] the round's unique seeds
  unsigned long long* cnt;  // [4] unique seeds of this round; due seeds, unique seeds, pops so far
  double* h_planes;         // [max_batch][p_max][4] the hull's outputs for a chunk
  int32_t* h_np;            // [max_batch]
  double* h_center;         // [max_batch][3]
  int32_t* h_rtn;           // [max_batch]
  int32_t *n_seg, *n_planes, *rtn;  // outputs, any may be null
  void *planes, *seeds, *centers;   // in the call's plane_dtype
};

// One wave per row.  Every lane holds the same Row and takes the same branches; the plane test of a polytope runs its planes over
// the lanes and one ballot decides.  In the first round the row is started: path_len and every voxel are validated (BAD_PATH).
__global__ __launch_bounds__(64) void k_corr_advance(CorrDev A, int first) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int len = A.path_len[row];
  const int32_t* path = A.path_xyz + (size_t)row * A.path_cap * 3;
  kc::Row r;
  if (first) {
    bool bad = len <= 0 || len > A.path_cap;
    if (!bad) {
      int out = 0;
      for (int i = lane; i < len; i += 64) out |= kc::voxel_inside(path + 3 * i, A.X, A.Y, A.Z) ? 0 : 1;
      bad = __any(out) != 0;
    }
    r = kc::row_start(bad);
  } else {
    r = A.rows[row];
  }
  if (r.state == kc::kWalking) {
    const double* planes = A.st_planes + (size_t)row * A.seg_cap * A.p_max * 4;
    const int32_t* np = A.st_np + (size_t)row * A.seg_cap;
    const int pops = r.pops;
    kc::advance(r, path, len, A.seg_cap, A.pop_back, A.res, A.lower, [&](int level, const double* cur) {
      const double* pl = planes + (size_t)level * A.p_max * 4;
      const int n = np[level];
      int ex = 0;
      for (int t = lane; t < n; t += 64) ex |= cc::plane_excludes(cur, pl + 4 * t) ? 1 : 0;
      return __any(ex) != 0;
    });
    if (lane == 0 && r.pops != pops) atomicAdd(A.cnt + 3, (unsigned long long)(r.pops - pops));
  } else if (!first) {
    return;
  }
  if (lane == 0) A.rows[row] = r;
}

// One workgroup of 1024 threads strides over the rows: the four steps of kc::unique_seeds with a barrier between them.  The owner
// table is reached with relaxed agent-scope atomics (fetch_min to claim, atomic loads to read); the barriers order the steps.
// Owners are compacted in row order, so the seed list - and with it the chunking - is the same whatever ran first.
__global__ __launch_bounds__(1024) void k_corr_unique(CorrDev A) {
  __shared__ int wsum[16];
  __shared__ int base_s, due_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto owner = [&](int v) { return __hip_atomic_load(&A.table[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  if (tid == 0) base_s = due_s = 0;
  __syncthreads();
  int mine = 0;
  for (int b = tid; b < A.batch; b += 1024)
    if (A.rows[b].state == kc::kDue) {
      __hip_atomic_fetch_min(&A.table[kc::voxel_index(A.rows[b].seed, A.Y, A.Z)], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      mine++;
    }
  if (mine) atomicAdd(&due_s, mine);
  __syncthreads();
  for (int b0 = 0; b0 < A.batch; b0 += 1024) {  // ordered compaction of the owners
    const int b = b0 + tid;
    const bool own = b < A.batch && A.rows[b].state == kc::kDue && owner(kc::voxel_index(A.rows[b].seed, A.Y, A.Z)) == b;
    const unsigned long long bal = __ballot(own);
    if (lane == 0) wsum[wv] = __popcll(bal);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wv; w++) off += wsum[w];
    off += __popcll(bal & ((1ull << lane) - 1ull));
    if (own) {
      for (int a = 0; a < 3; a++) A.seed_list[3 * off + a] = A.rows[b].seed[a];
      A.rows[b].slot = off;
    }
    __syncthreads();
    if (tid == 0)
      for (int w = 0; w < 16; w++) base_s += wsum[w];
    __syncthreads();
  }
  for (int b = tid; b < A.batch; b += 1024)
    if (A.rows[b].state == kc::kDue) {
      const int o = owner(kc::voxel_index(A.rows[b].seed, A.Y, A.Z));
      if (o != b) A.rows[b].slot = A.rows[o].slot;  // an owner's slot was written before the last barrier and is not written again
    }
  __syncthreads();
  for (int b = tid; b < A.batch; b += 1024)
    if (A.rows[b].state == kc::kDue)
      __hip_atomic_store(&A.table[kc::voxel_index(A.rows[b].seed, A.Y, A.Z)], kc::kNoOwner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) {
    A.cnt[0] = (unsigned long long)base_s;
    A.cnt[1] += (unsigned long long)due_s;
    A.cnt[2] += (unsigned long long)base_s;
  }
}

// After generation + hull of the seeds [lo, lo + n) of the seed list: element j of the handle's cluster storage and of the hull's
// outputs belongs to slot lo + j.  One wave per row; rows that are not due, or whose slot lies in another chunk, return at once.
__global__ __launch_bounds__(64) void k_corr_append(Dev D, CorrDev A, int lo, int n) {
  const int row = blockIdx.x, lane = threadIdx.x;
  kc::Row r = A.rows[row];
  if (r.state != kc::kDue || r.slot < lo || r.slot >= lo + n) return;
  const int j = r.slot - lo;
  const int np = A.h_np[j];
  const int code = kc::judge(D.el[j].rtn == DIRECT_CLUSTER_OK, A.h_rtn[j], np, A.p_max);
  if (code != kc::kOk) {
    kc::stop(r, code);
  } else {
    const size_t at = (size_t)row * A.seg_cap + r.depth;  // depth < seg_cap: advance() ends a row that would need more
    for (int q = lane; q < 4 * np; q += 64) A.st_planes[at * A.p_max * 4 + q] = A.h_planes[(size_t)j * A.p_max * 4 + q];
    if (lane == 0) {
      double cur[3];
      cc::index2coord(r.seed, A.res, A.lower, cur);
      A.st_np[at] = np;
      for (int a = 0; a < 3; a++) {
        A.st_seeds[3 * at + a] = cur[a];
        A.st_centers[3 * at + a] = A.h_center[3 * j + a];
      }
    }
    kc::push(r);
  }
  if (lane == 0) A.rows[row] = r;
}

template <typename Real>
__device__ __forceinline__ void corr_store(void* base, size_t at, double v) {
  if (base) ((Real*)base)[at] = (Real)v;  // float: one rounding of the double
}

// One workgroup per row: the stack becomes the row's outputs; everything from n_seg on, and every plane row from a polytope's
// n_planes on, is zero.  Outputs come from the stack only now because a pop makes a running output unsafe.
template <typename Real>
__global__ __launch_bounds__(256) void k_corr_emit(CorrDev A) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const kc::Row r = A.rows[row];
  const size_t seg0 = (size_t)row * A.seg_cap;
  const double* planes = A.st_planes + seg0 * A.p_max * 4;
  const int32_t* np = A.st_np + seg0;
  for (int k = tid; k < A.seg_cap; k += 256) {
    if (A.n_planes) A.n_planes[seg0 + k] = k < r.depth ? np[k] : 0;
    for (int a = 0; a < 3; a++) {
      corr_store<Real>(A.seeds, 3 * (seg0 + k) + a, k < r.depth ? A.st_seeds[3 * (seg0 + k) + a] : 0.0);
      corr_store<Real>(A.centers, 3 * (seg0 + k) + a, k < r.depth ? A.st_centers[3 * (seg0 + k) + a] : 0.0);
    }
  }
  if (A.planes)
    for (int q = tid; q < A.seg_cap * A.p_max * 4; q += 256)
      corr_store<Real>(A.planes, seg0 * A.p_max * 4 + q, kc::emit_plane(r, planes, np, A.p_max, q));
  if (tid == 0) {
    if (A.n_seg) A.n_seg[row] = r.depth;
    if (A.rtn) A.rtn[row] = r.code;
  }
}
