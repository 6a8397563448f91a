// Kernels of direct_cluster_grid_path_clear_batch (include/direct_cluster.h, "clearance-aware grid paths"): the tile visit and
// the read-back walk of grid_path.h with `Clear`, on the graph and with the cost of grid_path_clear_math.h.  Included from
// direct_cluster.hip inside its anonymous namespace, after grid_path.h: PathDev, PathClearDev, k_path_init, the workspace
// (fields, flags, counters), the protocol and the fixpoint argument are that file's.
#pragma once

__global__ __launch_bounds__(256) void k_path_clear_relax(PathDev P, PathClearDev C, int round) { path_visit<true, false>(P, C, nullptr, round); }

__global__ __launch_bounds__(64) void k_path_clear_trace(PathDev P, PathClearDev C, int rounds_done, int32_t* path_xyz, int32_t* path_len,
                                                         double* path_cost, int32_t* stats, int32_t* rtn, int32_t* path_d2,
                                                         int32_t* path_min_d2) {
  const int q = blockIdx.x;
  const int* e = P.ends + 6 * q;
  path_walk<true, false>(P, C, e, e + 3, P.field + (size_t)q * P.G, P.ring + (size_t)q * P.cap, C.ring_d2 + (size_t)q * P.cap, q, q,
                         rounds_done, PathOut{path_xyz, path_len, path_cost, rtn, path_d2, path_min_d2, stats});
}
