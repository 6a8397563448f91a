// Arithmetic of direct_cluster_grid_path_batch (include/direct_cluster.h, "grid paths"): the graph, the weights, the relaxation
// of one voxel from its 8^3 tile staged with a one-voxel halo, the acceptance rule with the pruning bound, which neighbouring
// tiles a changed voxel wakes, and the predecessor rule of the read-back.  Plain C++ behind a qualifier macro: the kernels of
// grid_path.h call these functions, and g++ compiles the same header for the CPU tests (tests/grid_path_harness.py).  The only
// floating-point operation is one double addition per candidate, so the two compilers produce the same bits.
//
// The graph is gridPathFinder::AstarSearch's (global_planner/src/utils/a_star.cpp:179-280): the 26 neighbours of a voxel
// (:224-234), a move goes INTO a voxel inside the map whose map byte is 0 (:236-246), no corner-cutting rule, and a move costs
// sqrt(dx^2 + dy^2 + dz^2) in double added to the gScore of the voxel it leaves (:252-254).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DIRECT_GRIDPATH_HD __host__ __device__ __forceinline__
#else
#define DIRECT_GRIDPATH_HD inline
#endif

namespace direct {
namespace gridpath {

constexpr int kTile = 8;                       // voxels per tile edge
constexpr int kTileVox = kTile * kTile * kTile;
constexpr int kHalo = kTile + 2;               // staged edge: the tile and one voxel around it
// Staged index of halo voxel (hx, hy, hz), each in [0, kHalo): hx * kStrideX + hy * kStrideY + hz.  The x stride is padded
// from 100 to 104 doubles: 104 = 8 (mod 32), so the 32 lanes (x 0..3, z 0..7) that one LDS cycle of an 8-byte read serves
// fall into 32 different 8-byte bank pairs, for every one of the 26 neighbour offsets (they shift all lanes alike).
constexpr int kStrideY = kHalo;
constexpr int kStrideX = 104;
constexpr int kStaged = kHalo * kStrideX;      // doubles of a staged tile (8320 B)
#ifndef DIRECT_GRIDPATH_LOCAL_ITERS
#define DIRECT_GRIDPATH_LOCAL_ITERS 64         // (a test build of the harness lowers it to reach the self-wake branch on small maps)
#endif
constexpr int kLocalIters = DIRECT_GRIDPATH_LOCAL_ITERS;  // sweeps of a tile per visit; a tile that is still changing then wakes itself

// sqrt(2.0) and sqrt(3.0) correctly rounded to double, written as bits so that no compiler's sqrt is involved
constexpr double kW1 = 1.0, kW2 = 0x1.6a09e667f3bcdp+0, kW3 = 0x1.bb67ae8584caap+0;

DIRECT_GRIDPATH_HD double inf() { return HUGE_VAL; }

// Neighbour k = 0 .. 25 in ascending (dx, dy, dz) lexicographic order from (-1, -1, -1), the centre left out.
DIRECT_GRIDPATH_HD void neighbour(int k, int& dx, int& dy, int& dz) {
  const int q = k < 13 ? k : k + 1;
  dx = q / 9 - 1;
  dy = (q / 3) % 3 - 1;
  dz = q % 3 - 1;
}
DIRECT_GRIDPATH_HD double weight(int dx, int dy, int dz) {
  const int n = (dx != 0) + (dy != 0) + (dz != 0);
  return n == 1 ? kW1 : (n == 2 ? kW2 : kW3);
}
DIRECT_GRIDPATH_HD double weight_of(int k) {
  int dx, dy, dz;
  neighbour(k, dx, dy, dz);
  return weight(dx, dy, dz);
}
DIRECT_GRIDPATH_HD int staged_index(int hx, int hy, int hz) { return hx * kStrideX + hy * kStrideY + hz; }

// min over the 26 neighbours u of fl(d(u) + w(u, v)) for the voxel staged at index c (an interior voxel: all 26 neighbours are
// staged; a neighbour outside the map or an obstacle holds +inf and contributes +inf)
DIRECT_GRIDPATH_HD double relax_candidate(const double* staged, int c) {
  double best = inf();
#if defined(__clang__)
#pragma unroll
#endif
  for (int q = 0; q < 27; q++) {
    if (q == 13) continue;
    const int dx = q / 9 - 1, dy = (q / 3) % 3 - 1, dz = q % 3 - 1;
    const double cand = staged[c + dx * kStrideX + dy * kStrideY + dz] + weight(dx, dy, dz);
    best = cand < best ? cand : best;
  }
  return best;
}
// A candidate replaces the voxel's value when it is smaller and not above the pruning bound (the value of the goal as the
// visit read it: every value is an upper bound of the true distance at all times, so a voxel beyond the bound cannot lie on
// a shortest path to the goal, and nothing at or below the final bound is ever refused).
DIRECT_GRIDPATH_HD bool accept(double cand, double cur, double bound) { return cand < cur && cand <= bound; }

// The neighbouring tiles that see the voxel at (lx, ly, lz) of a tile in their halo: bit (a * 9 + b * 3 + c) for the tile at
// offset (a - 1, b - 1, c - 1); bit 13 (the tile itself) is never set here.
DIRECT_GRIDPATH_HD unsigned wake_mask(int lx, int ly, int lz) {
  const unsigned mx = (lx == 0 ? 1u : 0u) | 2u | (lx == kTile - 1 ? 4u : 0u);
  const unsigned my = (ly == 0 ? 1u : 0u) | 2u | (ly == kTile - 1 ? 4u : 0u);
  const unsigned mz = (lz == 0 ? 1u : 0u) | 2u | (lz == kTile - 1 ? 4u : 0u);
  unsigned m = 0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++)
      for (int c = 0; c < 3; c++)
        if (((mx >> a) & 1u) && ((my >> b) & 1u) && ((mz >> c) & 1u)) m |= 1u << (a * 9 + b * 3 + c);
  return m & ~(1u << 13);
}

// Read-back: neighbour k (value du, +inf when it is outside the map) is a predecessor of a voxel of value dv when the one
// addition the relaxation made reproduces dv to the bit.  The path takes the lowest such k.
DIRECT_GRIDPATH_HD bool is_predecessor(double du, int k, double dv) { return du + weight_of(k) == dv; }

// the library's default for max_rounds == 0 (documented in the header): twice the number of tiles plus 64
DIRECT_GRIDPATH_HD int tiles_along(int n) { return (n + kTile - 1) / kTile; }
DIRECT_GRIDPATH_HD long long default_max_rounds(int max_x, int max_y, int max_z) {
  return 2LL * tiles_along(max_x) * tiles_along(max_y) * tiles_along(max_z) + 64;
}

}  // namespace gridpath
}  // namespace direct
