// Kernels of direct_cluster_grid_path_clear_batch (include/direct_cluster.h, "clearance-aware grid paths"): the tiled
// label-correcting relaxation of grid_path.h on the graph and with the cost of grid_path_clear_math.h.  Included from
// direct_cluster.hip inside its anonymous namespace, after grid_path.h: PathDev, k_path_init, the workspace (fields, flags,
// counters) and the protocol - one launch per round, every kernel ends on its own - are that file's and are not repeated here.
//
// What differs.  A lane loads, once per visit and per owned voxel, the voxel's stored D2 and, below n_pen, its table entry
// (plain global loads; the table is a small device array, the staged tile and its bank layout are untouched), and keeps "open"
// (byte 0 and D2 >= min_d2) and the penalty in registers for all sweeps: a sweep is relax_candidate + one addition + accept.
// The fixpoint argument carries over: every value is the fold of some walk, a -> fl(fl(a + w) + p) is monotone and
// >= a for w > 0 and p >= 0, so the field reaches the one fixpoint a heap Dijkstra computes with the same two additions, and
// pruning by the goal's current value stays valid.
#pragma once

struct PathClearDev {
  const int32_t* d2;   // [G] the handle's distance field
  const double* pen;   // [n_pen] the penalty table (null when n_pen is 0)
  int n_pen, min_d2;
  int* ring_d2;        // [max_batch][cap] read-back scratch beside PathDev::ring: the stored D2 of hop k at k % cap
};

// One round: k_path_relax with the floor and the penalty.  Same lane -> voxel map, same LDS, same wake protocol.
__global__ __launch_bounds__(256) void k_path_clear_relax(PathDev P, PathClearDev C, int round) {
  const int q = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  uint8_t* cur = P.flag[round & 1] + (size_t)q * P.ntiles;
  if (!cur[tile]) return;
  __shared__ double s[gp::kStaged];
  __shared__ unsigned s_wake;
  uint8_t* nxt = P.flag[(round + 1) & 1] + (size_t)q * P.ntiles;
  double* d = P.field + (size_t)q * P.G;
  const int iz = tile % P.tz, iy = (tile / P.tz) % P.ty, ix = tile / (P.tz * P.ty);
  const int bx = ix * gp::kTile, by = iy * gp::kTile, bz = iz * gp::kTile;
  const int* e = P.ends + 6 * q;
  const double bound = d[e[3] * P.YZ + e[4] * P.Z + e[5]];  // the goal's value (its own penalty included), once per visit
  const int glx = e[3] - bx, gly = e[4] - by, glz = e[5] - bz;
  const int gl = (glx >= 0 && glx < gp::kTile && gly >= 0 && gly < gp::kTile && glz >= 0 && glz < gp::kTile)
                     ? gp::staged_index(glx + 1, gly + 1, glz + 1) : -1;
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
    const int32_t dd = in ? C.d2[g[j]] : 0;
    open[j] = in && gp::clear_open(P.map[g[j]], dd, C.min_d2);  // the start's own byte, D2 and penalty are never needed: its 0
                                                               // cannot be improved
    pen[j] = open[j] ? gp::clear_penalty(C.pen, C.n_pen, dd) : 0.0;
  }
  __syncthreads();
  if (tid == 0) cur[tile] = 0;
#pragma unroll
  for (int j = 0; j < 2; j++) v0[j] = v[j] = s[c[j]];
  // the sweeps: grid_path.h's, DELIBERATE RACE included (see the comment there; the argument needs monotone updates only)
  int busy = 0;
  for (int it = 0; it < gp::kLocalIters; it++) {
    int changed = 0;
    const double lim = gl >= 0 ? s[gl] : bound;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const double cand = gp::clear_candidate(s, c[j], pen[j]);
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

// Read-back, one wave per query, as k_path_trace with the two-addition predecessor test.  Per hop the wave loads the current
// voxel's stored D2 (one address for all lanes) and, unless it is the start, its penalty, and carries the minimum of D2 over
// the voxels entered so far.  Hop k's voxel goes to ring[k % cap] and its D2 to ring_d2[k % cap].
__global__ __launch_bounds__(64) void k_path_clear_trace(PathDev P, PathClearDev C, int rounds_done, int32_t* path_xyz, int32_t* path_len,
                                                         double* path_cost, int32_t* stats, int32_t* rtn, int32_t* path_d2,
                                                         int32_t* path_min_d2) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int* e = P.ends + 6 * q;
  const double* d = P.field + (size_t)q * P.G;
  int* ring = P.ring + (size_t)q * P.cap;
  int* ring_d2 = C.ring_d2 + (size_t)q * P.cap;
  const int pend = P.pending[q];
  int code = DIRECT_GRID_PATH_OK, len = 0, min_d2 = DIRECT_DIST_NONE;
  double cost = __builtin_nan("");
  if (pend < 0) {
    code = DIRECT_GRID_PATH_BAD_ENDPOINT;
  } else if (pend == rounds_done) {
    code = DIRECT_GRID_PATH_ROUND_LIMIT;
  } else {
    int x = e[3], y = e[4], z = e[5];
    double dv = d[x * P.YZ + y * P.Z + z];
    cost = dv;
    if (!(dv < gp::inf())) {
      code = DIRECT_GRID_PATH_NO_PATH;
    } else {
      int dx, dy, dz;
      gp::neighbour(lane < 26 ? lane : 0, dx, dy, dz);
      for (;;) {  // dv falls with every hop (w >= 1, pen >= 0) and only the start holds 0: at most G hops
        const int idx = x * P.YZ + y * P.Z + z;
        const int32_t dd = C.d2[idx];
        if (lane == 0) {
          if (path_xyz) ring[len % P.cap] = idx;
          if (path_d2) ring_d2[len % P.cap] = dd;
        }
        len++;
        if ((x == e[0] && y == e[1] && z == e[2]) || len > P.G) break;
        min_d2 = dd < min_d2 ? dd : min_d2;
        const double pen = gp::clear_penalty(C.pen, C.n_pen, dd);
        const int ux = x + dx, uy = y + dy, uz = z + dz;
        const double du = (lane < 26 && path_inside(P, ux, uy, uz)) ? d[ux * P.YZ + uy * P.Z + uz] : gp::inf();
        const unsigned long long m = __ballot(lane < 26 && gp::clear_is_predecessor(du, lane, pen, dv));
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
  if ((path_xyz || path_d2) && len > 0) {
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
      if (path_d2) path_d2[(size_t)q * P.cap + i] = ring_d2[slot];
    }
  }
  if (lane == 0) {
    if (path_len) path_len[q] = len;
    if (path_cost) path_cost[q] = cost;
    if (rtn) rtn[q] = code;
    if (stats) { stats[2 * q] = P.rounds[q]; stats[2 * q + 1] = P.visits[q]; }
    if (path_min_d2) path_min_d2[q] = min_d2;
  }
}
