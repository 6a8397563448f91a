// Kernels of direct_cluster_grid_path_fan_batch (include/direct_cluster.h, "shared-start grid paths"): ONE field per source,
// any number of goals read back from it.  Included from direct_cluster.hip inside its anonymous namespace, after grid_path.h and
// grid_path_clear.h: PathDev, PathClearDev, k_path_init, the tile visit and the read-back walk (here with `Fan`), the workspace
// (fields, flags, counters) and the protocol - one launch per round, every kernel ends on its own - are grid_path.h's and are
// not repeated here.  A source takes the slot a query takes there (ends = (source, source) for k_path_init); each kernel is one
// template on `Clear`, the plain cost of grid_path_math.h or the floor and the two additions of grid_path_clear_math.h.
//
// What differs.  The field d depends on the start alone; the pairwise kernels read the goal only to prune.  Here the pruning
// bound of source s is bound[s] = max of d_s over its ELIGIBLE goals (grid_path_fan_math.h), made by k_fan_bound, one workgroup per
// source striding over its goals (grouped by the host, CSR) and reducing by shuffles: no floating-point atomics.  Costs never
// fall along a walk, so a voxel above that bound lies on no optimal path to any goal of s (grid_path.h's argument with "the worst
// goal").  The bound only falls from launch to launch, so the value a visit reads is valid however old.
#pragma once

struct FanDev {
  const int* goals;   // [n_goal][3]
  const int* gsrc;    // [n_goal] the source of each goal
  const int* order;   // [n_goal] goal indices grouped by source ...
  const int* off;     // [n_src + 1] ... the goals of source s are order[off[s] .. off[s + 1])
  double* bound;      // [n_src]
  int* ring;          // [n_goal][cap] read-back scratch per GOAL: linear voxel index of hop k at k % cap
  int* ring_d2;       // [n_goal][cap] the stored D2 of hop k (Clear with path_d2 only)
  int n_src, n_goal;
};

// bound[s], one workgroup of kFanBoundLanes per source: the lanes stride over the source's goals (each goal costs a chain of four
// dependent loads, so the width is what makes a refresh before every round cheap at thousands of goals), every wave reduces by
// shuffles, and the first wave reduces the waves' maxima through LDS
constexpr int kFanBoundLanes = 1024;
template <bool Clear>
__global__ __launch_bounds__(kFanBoundLanes) void k_fan_bound(PathDev P, PathClearDev C, FanDev F) {
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  __shared__ double s_max[kFanBoundLanes / 64];
  const int* e = P.ends + 6 * s;
  double m = 0.0;
  if (path_inside(P, e[0], e[1], e[2])) {
    const double* d = P.field + (size_t)s * P.G;
    const int end = F.off[s + 1];
    for (int i = F.off[s] + tid; i < end; i += kFanBoundLanes) {
      const int* g = F.goals + 3 * F.order[i];
      if (!path_inside(P, g[0], g[1], g[2])) continue;
      const int idx = g[0] * P.YZ + g[1] * P.Z + g[2];
      const bool self = g[0] == e[0] && g[1] == e[1] && g[2] == e[2];
      const int32_t dd = Clear ? C.d2[idx] : 0;
      if (gp::fan_eligible(self, P.map[idx], dd, Clear ? C.min_d2 : 0)) m = gp::fan_bound_fold(m, d[idx]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = gp::fan_bound_fold(m, __shfl_xor(m, o));
  if (lane == 0) s_max[tid >> 6] = m;
  __syncthreads();
  if (tid < 64) {
    m = tid < kFanBoundLanes / 64 ? s_max[tid] : 0.0;
#pragma unroll
    for (int o = kFanBoundLanes / 128; o > 0; o >>= 1) m = gp::fan_bound_fold(m, __shfl_xor(m, o));
    if (tid == 0) F.bound[s] = m;
  }
}

// One round over (tiles, sources): grid_path.h's tile visit with lim = bound[s], read once per visit (no goal-in-tile case)
template <bool Clear>
__global__ __launch_bounds__(256) void k_fan_relax(PathDev P, PathClearDev C, const double* bound, int round) {
  path_visit<Clear, true>(P, C, bound, round);
}

// Read-back, one wave per GOAL on the field of its source: grid_path.h's walk with the (source, goal) indirection and a ring per goal
template <bool Clear>
__global__ __launch_bounds__(64) void k_fan_trace(PathDev P, PathClearDev C, FanDev F, int rounds_done, int32_t* path_xyz, int32_t* path_len,
                                                  double* path_cost, int32_t* rtn, int32_t* path_d2, int32_t* path_min_d2) {
  const int q = blockIdx.x, src = F.gsrc[q];
  path_walk<Clear, true>(P, C, P.ends + 6 * src, F.goals + 3 * q, P.field + (size_t)src * P.G, F.ring + (size_t)q * P.cap,
                         F.ring_d2 + (size_t)q * P.cap, q, src, rounds_done,
                         PathOut{path_xyz, path_len, path_cost, rtn, path_d2, path_min_d2, nullptr});
}

// stats[s] = (rounds in which source s had an active tile, its tile visits): per source, so not the trace's to write
__global__ __launch_bounds__(64) void k_fan_stats(PathDev P, int n_src, int32_t* stats) {
  for (int s = threadIdx.x; s < n_src; s += 64) {
    stats[2 * s] = P.rounds[s];
    stats[2 * s + 1] = P.visits[s];
  }
}
