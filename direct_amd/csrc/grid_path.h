// Kernels of direct_cluster_grid_path_batch (include/direct_cluster.h, "grid paths"): optimal 26-connected voxel paths for a
// batch of (start, goal) queries on the handle's map, by a tiled label-correcting relaxation.  Included from
// direct_cluster.hip inside its anonymous namespace; the arithmetic is grid_path_math.h (plain C++, also compiled by g++ for
// tests/test_grid_path_restatement.py).  The tile visit (path_visit) and the read-back walk (path_walk) are written ONCE here,
// templated on `Clear` (the floor and the penalty of grid_path_clear_math.h) and `Fan` (one field per source, grid_path_fan.h);
// the kernels of the three entry points are wrappers of a line or two, here, in grid_path_clear.h and in grid_path_fan.h.
//
// Per query a field d of doubles over the map, d(start) = 0 and +inf elsewhere, and one "active" byte per 8^3 tile.  A ROUND
// is one launch of a relax kernel over (tiles, queries): the workgroup of an active tile stages the tile with its halo in LDS,
// sweeps it until nothing changes, writes the changed values back and wakes the neighbouring tiles that border a changed
// voxel for the NEXT round (two flag arrays, used in turn).  Every value is at all times the cost of some walk from the
// start, hence an upper bound of the true distance, and rounded addition of a positive weight is monotone - as is, with a
// penalty p >= 0, the two-addition step a -> fl(fl(a + w) + p), which is also >= a for w > 0: whatever order the tiles run in
// and whichever of a neighbour's old or new values a tile reads, the field reaches the one fixpoint a heap Dijkstra computes
// with the same additions.  Costs never fall along a walk, so a voxel above the value of the goal - of the
// WORST eligible goal where a field serves many (bound[s], grid_path_fan.h) - lies on no optimal path and is pruned; that value
// only falls, so any reading of it, however old, is a valid bound.  An 8-byte aligned store is one instruction, so a value read
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

// what `Clear` reads (all zero and never read without it)
struct PathClearDev {
  const int32_t* d2;   // [G] the handle's distance field
  const double* pen;   // [n_pen] the penalty table (null when n_pen is 0)
  int n_pen, min_d2;
  int* ring_d2;        // [max_batch][cap] read-back scratch beside PathDev::ring: the stored D2 of hop k at k % cap
};

// the outputs of a read-back, each skipped when null; path_d2 and path_min_d2 are `Clear`'s, stats the pairwise kernels'
struct PathOut {
  int32_t *path_xyz, *path_len;
  double* path_cost;
  int32_t *rtn, *path_d2, *path_min_d2, *stats;
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

// One tile visit of one round.  Workgroup (tile, query), 256 lanes: lane t owns the voxels (x4, y, z) and (x4 + 4, y, z) of the
// tile with z = t & 7, x4 = (t >> 3) & 3, y = t >> 5, so that the 32 lanes of one LDS cycle differ in (x4, z) only
// (grid_path_math.h, kStrideX).  Each lane writes only its own two voxels: no write conflicts, no floating-point atomics.
// What the template parameters decide, and nothing else:
//   lim   !Fan: the goal's value (its own penalty included), read once per visit - unless the goal lies in this tile: then every
//         sweep takes the staged value.  Fan: fan_bound[q], the worst eligible goal's value as the last k_fan_bound saw it.
//   open  a move goes INTO a free voxel of the map; Clear: whose stored D2 is at least min_d2 as well.
//   pen   Clear: the voxel's table entry, loaded once per visit (plain global loads) and kept in a register for all sweeps, so
//         that a sweep is relax_candidate + one addition + accept; otherwise none.
// The start's own byte, D2 and penalty are never needed: its 0 cannot be improved.
template <bool Clear, bool Fan>
__device__ __forceinline__ void path_visit(const PathDev& P, const PathClearDev& C, const double* fan_bound, int round) {
  const int q = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  uint8_t* cur = P.flag[round & 1] + (size_t)q * P.ntiles;
  if (!cur[tile]) return;
  __shared__ double s[gp::kStaged];
  __shared__ unsigned s_wake;
  uint8_t* nxt = P.flag[(round + 1) & 1] + (size_t)q * P.ntiles;
  double* d = P.field + (size_t)q * P.G;
  const int iz = tile % P.tz, iy = (tile / P.tz) % P.ty, ix = tile / (P.tz * P.ty);
  const int bx = ix * gp::kTile, by = iy * gp::kTile, bz = iz * gp::kTile;
  double bound;
  int gl = -1;  // the goal's staged index when it lies in this tile
  if (Fan) {
    bound = fan_bound[q];
  } else {
    const int* e = P.ends + 6 * q;
    bound = d[e[3] * P.YZ + e[4] * P.Z + e[5]];
    const int glx = e[3] - bx, gly = e[4] - by, glz = e[5] - bz;
    if (glx >= 0 && glx < gp::kTile && gly >= 0 && gly < gp::kTile && glz >= 0 && glz < gp::kTile)
      gl = gp::staged_index(glx + 1, gly + 1, glz + 1);
  }
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
  if (tid == 0) cur[tile] = 0;  // every wave has read the byte (barrier above) and only this workgroup looks at it in this
                                // round; the next round of this parity may set it again
#pragma unroll
  for (int j = 0; j < 2; j++) v0[j] = v[j] = s[c[j]];
  // DELIBERATE RACE inside a sweep: a lane reads s[] (its 26 neighbours, and s[gl] as the bound) while other lanes store to their
  // own entries, with no barrier in between.  The algorithm allows it (either value is an upper bound of the true distance, the
  // updates are monotone, and an aligned 8-byte LDS store is one instruction, so a value is never torn); formally it is a data
  // race on a plain __shared__ array.  What the code relies on: the vote that ends every sweep is a barrier AND a
  // compiler fence, so s[] is loaded afresh in every sweep and each sweep sees at least everything stored before the previous
  // barrier - which is all the termination test needs (a sweep in which no lane changed anything read a quiescent s[]).
  int busy = 0;
  for (int it = 0; it < gp::kLocalIters; it++) {
    int changed = 0;
    const double lim = gl >= 0 ? s[gl] : bound;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const double cand = Clear ? gp::clear_candidate(s, c[j], pen[j]) : gp::relax_candidate(s, c[j]);
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

// Read-back of one path by one wave, goal -> start on field d: lanes 0 .. 25 test the 26 neighbours of the current voxel, the
// lowest matching lane is the predecessor.  Hop k (the goal is hop 0) goes to ring[k % cap]; when the start is reached after L
// voxels the last min(L, cap) hops - the FIRST voxels of the path - are still there and are emitted start -> goal into output
// slot q.  Clear: the two-addition predecessor test; per hop the wave loads the current voxel's stored D2 (one address for all
// lanes, to ring_d2[k % cap]) and, unless it is the start, its penalty, and carries the minimum of D2 over the voxels entered.
// src is the workspace slot the field belongs to: q itself for a pair, the goal's source for a fan, where the field is only
// read (any number of goals may walk it at once), the endpoints are tested here (k_path_init saw the source alone) and the
// statistics, being per source, are k_fan_stats's to write.
template <bool Clear, bool Fan>
__device__ __forceinline__ void path_walk(const PathDev& P, const PathClearDev& C, const int* start, const int* goal, const double* d,
                                          int* ring, int* ring_d2, int q, int src, int rounds_done, const PathOut& o) {
  const int lane = threadIdx.x;
  const int pend = P.pending[src];
  const bool want_d2 = Clear && o.path_d2;
  int code = DIRECT_GRID_PATH_OK, len = 0, min_d2 = DIRECT_DIST_NONE;
  double cost = __builtin_nan("");
  if (Fan ? !path_inside(P, start[0], start[1], start[2]) || !path_inside(P, goal[0], goal[1], goal[2]) : pend < 0) {
    code = DIRECT_GRID_PATH_BAD_ENDPOINT;
  } else if (pend == rounds_done) {
    code = DIRECT_GRID_PATH_ROUND_LIMIT;
  } else {
    int x = goal[0], y = goal[1], z = goal[2];
    double dv = d[x * P.YZ + y * P.Z + z];
    cost = dv;
    if (!(dv < gp::inf())) {
      code = DIRECT_GRID_PATH_NO_PATH;
    } else {
      int dx, dy, dz;
      gp::neighbour(lane < 26 ? lane : 0, dx, dy, dz);
      for (;;) {  // dv falls with every hop (w >= 1, pen >= 0) and only the start holds 0: at most G hops
        const int idx = x * P.YZ + y * P.Z + z;
        const int32_t dd = Clear ? C.d2[idx] : 0;
        if (lane == 0) {
          if (o.path_xyz) ring[len % P.cap] = idx;
          if (want_d2) ring_d2[len % P.cap] = dd;
        }
        len++;
        if ((x == start[0] && y == start[1] && z == start[2]) || len > P.G) break;
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
  if ((o.path_xyz || want_d2) && len > 0) {
    __threadfence();
    __syncthreads();  // one wave: lane 0's ring stores come before the other lanes' reads below
    const int n = len < P.cap ? len : P.cap;
    for (int i = lane; i < n; i += 64) {
      const int slot = (len - 1 - i) % P.cap;
      if (o.path_xyz) {
        const int idx = ring[slot];
        int32_t* xyz = o.path_xyz + ((size_t)q * P.cap + i) * 3;
        xyz[0] = idx / P.YZ; xyz[1] = (idx / P.Z) % P.Y; xyz[2] = idx % P.Z;
      }
      if (want_d2) o.path_d2[(size_t)q * P.cap + i] = ring_d2[slot];
    }
  }
  if (lane == 0) {
    if (o.path_len) o.path_len[q] = len;
    if (o.path_cost) o.path_cost[q] = cost;
    if (o.rtn) o.rtn[q] = code;
    if (!Fan && o.stats) { o.stats[2 * q] = P.rounds[src]; o.stats[2 * q + 1] = P.visits[src]; }
    if (Clear && o.path_min_d2) o.path_min_d2[q] = min_d2;
  }
}

// the plain pair (direct_cluster_grid_path_batch): one round over (tiles, queries), and the read-back, one wave per query
__global__ __launch_bounds__(256) void k_path_relax(PathDev P, int round) { path_visit<false, false>(P, PathClearDev{}, nullptr, round); }

__global__ __launch_bounds__(64) void k_path_trace(PathDev P, int rounds_done, int32_t* path_xyz, int32_t* path_len, double* path_cost,
                                                   int32_t* stats, int32_t* rtn) {
  const int q = blockIdx.x;
  const int* e = P.ends + 6 * q;
  path_walk<false, false>(P, PathClearDev{}, e, e + 3, P.field + (size_t)q * P.G, P.ring + (size_t)q * P.cap, nullptr, q, q, rounds_done,
                          PathOut{path_xyz, path_len, path_cost, rtn, nullptr, nullptr, stats});
}
