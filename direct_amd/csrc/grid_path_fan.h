// Kernels of direct_cluster_grid_path_fan_batch (include/direct_cluster.h, "shared-start grid paths"): ONE field per source,
// any number of goals read back from it.  Included from direct_cluster.hip inside its anonymous namespace, after grid_path.h and
// grid_path_clear.h: PathDev, PathClearDev, k_path_init, the workspace (fields, flags, counters) and the protocol - one launch
// per round, every kernel ends on its own - are those files' and are not repeated here.  A source takes the slot a query takes
// there (ends = (source, source) for k_path_init); each kernel is one template on `Clear`, the plain cost of grid_path_math.h or
// the floor and the two additions of grid_path_clear_math.h.
//
// What differs.  The field d depends on the start alone; the pairwise kernels read the goal only to prune.  Here the pruning
// bound of source s is bound[s] = max of d_s over its ELIGIBLE goals (grid_path_fan_math.h), made by k_fan_bound, one workgroup per
// source striding over its goals (grouped by the host, CSR) and reducing by shuffles: no floating-point atomics.  Costs never
// fall along a walk, so a voxel above that bound lies on no optimal path to any goal of s: 6.16's argument with "the goal"
// replaced by "the worst goal".  The bound only falls from launch to launch, so the value a visit reads is valid however old.
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

// One round: k_path_relax / k_path_clear_relax over (tiles, sources) with lim = bound[s], read once per visit.  Same lane ->
// voxel map, same LDS and bank layout, same wake protocol; the goal-in-tile special case is gone.
template <bool Clear>
__global__ __launch_bounds__(256) void k_fan_relax(PathDev P, PathClearDev C, const double* bound, int round) {
  const int q = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  uint8_t* cur = P.flag[round & 1] + (size_t)q * P.ntiles;
  if (!cur[tile]) return;
  __shared__ double s[gp::kStaged];
  __shared__ unsigned s_wake;
  uint8_t* nxt = P.flag[(round + 1) & 1] + (size_t)q * P.ntiles;
  double* d = P.field + (size_t)q * P.G;
  const int iz = tile % P.tz, iy = (tile / P.tz) % P.ty, ix = tile / (P.tz * P.ty);
  const int bx = ix * gp::kTile, by = iy * gp::kTile, bz = iz * gp::kTile;
  const double lim = bound[q];  // the worst eligible goal's value as the last k_fan_bound saw it
  if (tid == 0) {
    s_wake = 0u;
    P.rounds[q] = round + 1;
    atomicAdd(&P.visits[q], 1);
  }
  for (int i = tid; i < gp::kHalo * gp::kHalo * gp::kHalo; i += 256) {
    const int hz = i % gp::kHalo, hy = (i / gp::kHalo) % gp::kHalo, hx = i / (gp::kHalo * gp::kHalo);
    const int x = bx + hx - 1, y = by + hy - 1, z = bz + hz - 1;
    s[gp::staged_index(hx, hy, hz)] = path_inside(P, x, y, z) ? d[x * P.YZ + y * P.Z + z] : gp::inf();
  }
  const int lz = tid & 7, lx0 = (tid >> 3) & 3, ly = tid >> 5;
  int c[2], g[2];
  bool open[2];
  double pen[2], v0[2], v[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int lx = lx0 + 4 * j, x = bx + lx, y = by + ly, z = bz + lz;
    c[j] = gp::staged_index(lx + 1, ly + 1, lz + 1);
    const bool in = path_inside(P, x, y, z);
    g[j] = in ? x * P.YZ + y * P.Z + z : 0;
    if (Clear) {
      const int32_t dd = in ? C.d2[g[j]] : 0;
      open[j] = in && gp::clear_open(P.map[g[j]], dd, C.min_d2);
      pen[j] = open[j] ? gp::clear_penalty(C.pen, C.n_pen, dd) : 0.0;
    } else {
      open[j] = in && P.map[g[j]] == 0;
      pen[j] = 0.0;
    }
  }
  __syncthreads();
  if (tid == 0) cur[tile] = 0;  // as k_path_relax: every wave has read the byte, only this workgroup looks at it in this round
#pragma unroll
  for (int j = 0; j < 2; j++) v0[j] = v[j] = s[c[j]];
  // the sweeps: grid_path.h's, DELIBERATE RACE included (see the comment there; the argument needs monotone updates only)
  int busy = 0;
  for (int it = 0; it < gp::kLocalIters; it++) {
    int changed = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const double cand = Clear ? gp::clear_candidate(s, c[j], pen[j]) : gp::relax_candidate(s, c[j]);
      if (open[j] && gp::accept(cand, v[j], lim)) {
        v[j] = cand;
        s[c[j]] = cand;
        changed = 1;
      }
    }
    busy = __syncthreads_or(changed);
    if (!busy) break;
  }
  unsigned wake = 0u;
#pragma unroll
  for (int j = 0; j < 2; j++)
    if (v[j] != v0[j]) {
      d[g[j]] = v[j];
      wake |= gp::wake_mask(lx0 + 4 * j, ly, lz);
    }
  if (busy) wake |= 1u << 13;
  if (wake) atomicOr(&s_wake, wake);
  __syncthreads();
  const unsigned all = s_wake;
  if (tid < 27 && ((all >> tid) & 1u)) {
    const int nx = ix + tid / 9 - 1, ny = iy + (tid / 3) % 3 - 1, nz = iz + tid % 3 - 1;
    if (nx >= 0 && nx < P.tx && ny >= 0 && ny < P.ty && nz >= 0 && nz < P.tz) {
      nxt[(nx * P.ty + ny) * P.tz + nz] = 1;
      P.pending[q] = round + 1;
    }
  }
}

// Read-back, one wave per GOAL on the field of its source: k_path_trace / k_path_clear_trace with the (source, goal)
// indirection and a ring per goal.  The field is only read, so any number of goals may walk one field at once.
template <bool Clear>
__global__ __launch_bounds__(64) void k_fan_trace(PathDev P, PathClearDev C, FanDev F, int rounds_done, int32_t* path_xyz, int32_t* path_len,
                                                  double* path_cost, int32_t* rtn, int32_t* path_d2, int32_t* path_min_d2) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int src = F.gsrc[q];
  const int* e = P.ends + 6 * src;
  const int* gl = F.goals + 3 * q;
  const double* d = P.field + (size_t)src * P.G;
  int* ring = F.ring + (size_t)q * P.cap;
  int* ring_d2 = F.ring_d2 + (size_t)q * P.cap;
  int code = DIRECT_GRID_PATH_OK, len = 0, min_d2 = DIRECT_DIST_NONE;
  double cost = __builtin_nan("");
  if (!path_inside(P, e[0], e[1], e[2]) || !path_inside(P, gl[0], gl[1], gl[2])) {
    code = DIRECT_GRID_PATH_BAD_ENDPOINT;
  } else if (P.pending[src] == rounds_done) {
    code = DIRECT_GRID_PATH_ROUND_LIMIT;
  } else {
    int x = gl[0], y = gl[1], z = gl[2];
    double dv = d[x * P.YZ + y * P.Z + z];
    cost = dv;
    if (!(dv < gp::inf())) {
      code = DIRECT_GRID_PATH_NO_PATH;
    } else {
      int dx, dy, dz;
      gp::neighbour(lane < 26 ? lane : 0, dx, dy, dz);
      for (;;) {  // dv falls with every hop (w >= 1, pen >= 0) and only the source holds 0: at most G hops
        const int idx = x * P.YZ + y * P.Z + z;
        const int32_t dd = Clear ? C.d2[idx] : 0;
        if (lane == 0) {
          if (path_xyz) ring[len % P.cap] = idx;
          if (Clear && path_d2) ring_d2[len % P.cap] = dd;
        }
        len++;
        if ((x == e[0] && y == e[1] && z == e[2]) || len > P.G) break;
        min_d2 = Clear && dd < min_d2 ? dd : min_d2;
        const double pen = Clear ? gp::clear_penalty(C.pen, C.n_pen, dd) : 0.0;
        const int ux = x + dx, uy = y + dy, uz = z + dz;
        const double du = (lane < 26 && path_inside(P, ux, uy, uz)) ? d[ux * P.YZ + uy * P.Z + uz] : gp::inf();
        const unsigned long long m =
            __ballot(lane < 26 && (Clear ? gp::clear_is_predecessor(du, lane, pen, dv) : gp::is_predecessor(du, lane, dv)));
        if (!m) { len = P.G + 1; break; }  // cannot happen on a converged field
        const int k = __ffsll((long long)m) - 1;
        dv = __shfl(du, k);
        int kx, ky, kz;
        gp::neighbour(k, kx, ky, kz);
        x += kx; y += ky; z += kz;
      }
      if (len > P.G) {  // guard of the loop above: reported as "no path", never a hang
        code = DIRECT_GRID_PATH_NO_PATH;
        len = 0;
        cost = gp::inf();
        min_d2 = DIRECT_DIST_NONE;
      } else if (len > P.cap) {
        code = DIRECT_GRID_PATH_OVERFLOW;
      }
    }
  }
  if ((path_xyz || (Clear && path_d2)) && len > 0) {
    __threadfence();
    __syncthreads();  // one wave: lane 0's ring stores come before the other lanes' reads below
    const int n = len < P.cap ? len : P.cap;
    for (int i = lane; i < n; i += 64) {
      const int slot = (len - 1 - i) % P.cap;
      if (path_xyz) {
        const int idx = ring[slot];
        int32_t* o = path_xyz + ((size_t)q * P.cap + i) * 3;
        o[0] = idx / P.YZ; o[1] = (idx / P.Z) % P.Y; o[2] = idx % P.Z;
      }
      if (Clear && path_d2) path_d2[(size_t)q * P.cap + i] = ring_d2[slot];
    }
  }
  if (lane == 0) {
    if (path_len) path_len[q] = len;
    if (path_cost) path_cost[q] = cost;
    if (rtn) rtn[q] = code;
    if (Clear && path_min_d2) path_min_d2[q] = min_d2;
  }
}

// stats[s] = (rounds in which source s had an active tile, its tile visits): per source, so not the trace's to write
__global__ __launch_bounds__(64) void k_fan_stats(PathDev P, int n_src, int32_t* stats) {
  for (int s = threadIdx.x; s < n_src; s += 64) {
    stats[2 * s] = P.rounds[s];
    stats[2 * s + 1] = P.visits[s];
  }
}
