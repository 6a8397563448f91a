// Kernels of direct_cluster_grid_path_batch (include/direct_cluster.h, "grid paths"): optimal 26-connected voxel paths for a
// batch of (start, goal) queries on the handle's map, by a tiled label-correcting relaxation.  Included from
// direct_cluster.hip inside its anonymous namespace; the arithmetic is grid_path_math.h (plain C++, also compiled by g++ for
// tests/test_grid_path_restatement.py).
//
// Per query a field d of doubles over the map, d(start) = 0 and +inf elsewhere, and one "active" byte per 8^3 tile.  A ROUND
// is one launch of k_path_relax over (tiles, queries): the workgroup of an active tile stages the tile with its halo in LDS,
// sweeps it until nothing changes, writes the changed values back and wakes the neighbouring tiles that border a changed
// voxel for the NEXT round (two flag arrays, used in turn).  Every value is at all times the cost of some walk from the
// start, hence an upper bound of the true distance, and rounded addition of a positive weight is monotone: whatever order
// the tiles run in and whichever of a neighbour's old or new values a tile reads, the field reaches the one fixpoint a heap
// Dijkstra computes with the same additions.  An 8-byte aligned store is one instruction, so a value read
// while its tile rewrites it is the old or the new one; plain stores are visible to the next launch on the stream.  No kernel
// waits for another workgroup: each ends on its own whatever the data.
#pragma once

namespace gp = direct::gridpath;

struct PathDev {
  int X, Y, Z, YZ, G;        // map dimensions, as Dev's
  int tx, ty, tz, ntiles;    // tiles per axis, tile t = (ix * ty + iy) * tz + iz
  const uint8_t* map;        // [G]
  double* field;             // [max_batch][G]
  uint8_t* flag[2];          // [max_batch][ntiles] tile active in a round of this parity
  int* ends;                 // [max_batch][6] start, goal
  int* pending;              // [max_batch] r + 1 of the last round r that woke a tile (0 after init; -1: bad endpoint)
  int* rounds;               // [max_batch] r + 1 of the last round in which a tile of the query ran
  int* visits;               // [max_batch] tile visits
  int* ring;                 // [max_batch][cap] read-back scratch: linear voxel index of hop k at k % cap
  int cap;
};

__device__ __forceinline__ bool path_inside(const PathDev& P, int x, int y, int z) {
  return x >= 0 && x < P.X && y >= 0 && y < P.Y && z >= 0 && z < P.Z;
}

// field <- +inf, 0 at the start; the start's tile active in round 0; counters
__global__ __launch_bounds__(256) void k_path_init(PathDev P) {
  const int q = blockIdx.y;
  const int* e = P.ends + 6 * q;
  const bool ok = path_inside(P, e[0], e[1], e[2]) && path_inside(P, e[3], e[4], e[5]);
  const int sidx = ok ? e[0] * P.YZ + e[1] * P.Z + e[2] : -1;
  const int stile = ok ? ((e[0] / gp::kTile) * P.ty + e[1] / gp::kTile) * P.tz + e[2] / gp::kTile : -1;
  double* d = P.field + (size_t)q * P.G;
  const int stride = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
  for (int i = t0; i < P.G; i += stride) d[i] = i == sidx ? 0.0 : gp::inf();
  for (int t = t0; t < P.ntiles; t += stride) {
    P.flag[0][(size_t)q * P.ntiles + t] = t == stile ? 1 : 0;
    P.flag[1][(size_t)q * P.ntiles + t] = 0;
  }
  if (t0 == 0) {
    P.pending[q] = ok ? 0 : -1;
    P.rounds[q] = 0;
    P.visits[q] = 0;
  }
}

// One round.  Workgroup (tile, query), 256 lanes: lane t owns the voxels (x4, y, z) and (x4 + 4, y, z) of the tile with
// z = t & 7, x4 = (t >> 3) & 3, y = t >> 5, so that the 32 lanes of one LDS cycle differ in (x4, z) only (grid_path_math.h,
// kStrideX).  Each lane writes only its own two voxels: no write conflicts, no floating-point atomics.
__global__ __launch_bounds__(256) void k_path_relax(PathDev P, int round) {
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
  const double bound = d[e[3] * P.YZ + e[4] * P.Z + e[5]];  // the goal's value, once per visit
  // ... unless the goal lies in this tile: then every sweep takes the staged value (any reading of it is a valid bound)
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
  double v0[2], v[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int lx = lx0 + 4 * j, x = bx + lx, y = by + ly, z = bz + lz;
    c[j] = gp::staged_index(lx + 1, ly + 1, lz + 1);
    const bool in = path_inside(P, x, y, z);
    g[j] = in ? x * P.YZ + y * P.Z + z : 0;
    open[j] = in && P.map[g[j]] == 0;  // a move goes INTO a free voxel of the map (the start's own byte is never needed:
                                       // its 0 cannot be improved)
  }
  __syncthreads();
  if (tid == 0) cur[tile] = 0;  // every wave has read the byte (barrier above) and only this workgroup looks at it in this
                                // round; the next round of this parity may set it again
#pragma unroll
  for (int j = 0; j < 2; j++) v0[j] = v[j] = s[c[j]];
  // DELIBERATE RACE inside a sweep: a lane reads s[] (its 26 neighbours, and s[gl] as the bound) while other lanes store to their
  // own entries, with no barrier in between.  The algorithm allows it (either value is an upper bound of the true distance, and
  // an aligned 8-byte LDS store is one instruction, so a value is never torn); formally it is a data race on a plain __shared__
  // array.  What the code relies on: __syncthreads_or at the end of every sweep is a barrier AND a compiler fence, so s[] is
  // loaded afresh in every sweep and each sweep sees at least everything stored before the previous barrier - which is all the
  // termination test needs (a sweep in which no lane changed anything read a quiescent s[]).
  int busy = 0;
  for (int it = 0; it < gp::kLocalIters; it++) {
    int changed = 0;
    const double lim = gl >= 0 ? s[gl] : bound;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const double cand = gp::relax_candidate(s, c[j]);
      if (open[j] && gp::accept(cand, v[j], lim)) {
        v[j] = cand;
        s[c[j]] = cand;  // other lanes may read the old or the new value in this sweep: both are upper bounds
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
  if (busy) wake |= 1u << 13;  // the sweeps ran out with changes left: the tile goes on in the next round
  if (wake) atomicOr(&s_wake, wake);
  __syncthreads();
  const unsigned all = s_wake;
  if (tid < 27 && ((all >> tid) & 1u)) {
    const int nx = ix + tid / 9 - 1, ny = iy + (tid / 3) % 3 - 1, nz = iz + tid % 3 - 1;
    if (nx >= 0 && nx < P.tx && ny >= 0 && ny < P.ty && nz >= 0 && nz < P.tz) {
      nxt[(nx * P.ty + ny) * P.tz + nz] = 1;  // plain stores of the same 1 / the same round number from several workgroups
      P.pending[q] = round + 1;
    }
  }
}

// Read-back, one wave per query: lanes 0 .. 25 test the 26 neighbours of the current voxel, the lowest matching lane is the
// predecessor.  Hop k (the goal is hop 0) goes to ring[k % cap]; when the start is reached after L voxels the last
// min(L, cap) hops - the FIRST voxels of the path - are still there and are emitted start -> goal.
__global__ __launch_bounds__(64) void k_path_trace(PathDev P, int rounds_done, int32_t* path_xyz, int32_t* path_len, double* path_cost,
                                                   int32_t* stats, int32_t* rtn) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int* e = P.ends + 6 * q;
  const double* d = P.field + (size_t)q * P.G;
  int* ring = P.ring + (size_t)q * P.cap;
  const int pend = P.pending[q];
  int code = DIRECT_GRID_PATH_OK, len = 0;
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
      for (;;) {  // dv falls with every hop and only the start holds 0: at most G hops
        if (path_xyz && lane == 0) ring[len % P.cap] = x * P.YZ + y * P.Z + z;
        len++;
        if ((x == e[0] && y == e[1] && z == e[2]) || len > P.G) break;
        const int ux = x + dx, uy = y + dy, uz = z + dz;
        const double du = (lane < 26 && path_inside(P, ux, uy, uz)) ? d[ux * P.YZ + uy * P.Z + uz] : gp::inf();
        const unsigned long long m = __ballot(lane < 26 && gp::is_predecessor(du, lane, dv));
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
      } else if (len > P.cap) {
        code = DIRECT_GRID_PATH_OVERFLOW;
      }
    }
  }
  if (path_xyz && len > 0) {
    __threadfence();
    __syncthreads();  // one wave: lane 0's ring stores come before the other lanes' reads below
    const int n = len < P.cap ? len : P.cap;
    for (int i = lane; i < n; i += 64) {
      const int idx = ring[(len - 1 - i) % P.cap];
      int32_t* o = path_xyz + ((size_t)q * P.cap + i) * 3;
      o[0] = idx / P.YZ; o[1] = (idx / P.Z) % P.Y; o[2] = idx % P.Z;
    }
  }
  if (lane == 0) {
    if (path_len) path_len[q] = len;
    if (path_cost) path_cost[q] = cost;
    if (rtn) rtn[q] = code;
    if (stats) { stats[2 * q] = P.rounds[q]; stats[2 * q + 1] = P.visits[q]; }
  }
}
