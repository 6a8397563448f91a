// Arithmetic of direct_cluster_cube_corridor_batch (include/direct_cluster.h, "cube corridors"): the cube of a voxel, the six
// planes and the centre of a cube, and the walk that selects the cubes of a grid path.  Plain C++ behind a qualifier macro: the
// kernels of cube_corridor.h call these functions, and g++ compiles the same header for the CPU tests
// (tests/cube_corridor_harness.py).  Every floating-point expression is double, written with plain * and +, contraction off.
//
// This is the corridor of the reference with is_cluster_on == false: paramSet then sets (itr_inflate_max, itr_cluster_max) =
// (1000, 0) (polyhedron_generator/src/cluster_server_cpu.cpp:91-97) and a polytope is the inflated cube of its seed voxel alone,
// a pure function of the seed and the map.
//
// THE MAP.  The slab test is one query of the summed-area table of the handle (obstacles in a box), and the table counts map
// bytes == 1, while cubeInflation_cpu tests bytes > 0.  The call is DEFINED on the table; it equals the reference's cube for
// maps whose bytes are 0 or 1, which is all direct_cluster_map_from_cloud produces (direct_cluster_set_map does not validate).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DIRECT_CUBECOR_HD __host__ __device__ __forceinline__
#else
#define DIRECT_CUBECOR_HD inline
#ifndef HULL_HD
#define HULL_HD inline
#endif
#endif
#if defined(__clang__)
#define DIRECT_CUBECOR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DIRECT_CUBECOR_NO_CONTRACT
#endif

#include "hull_core.h"

namespace direct {
namespace cubecor {

constexpr int kPlanes = 6;
constexpr int kNoCube = -1;  // c[0] of a slot that has no cube (beyond the path, or a voxel outside the map)

// ---- the cube of a voxel: cubeInflation_cpu (cluster_server_cpu.cpp:257-293) as k_inflate of direct_cluster.hip restates it -----
// c = (lo x, lo y, lo z, hi x, hi y, hi z), inclusive voxel indices.  obstacles(x0, y0, z0, x1, y1, z1) is the number of
// obstacle voxels in that inclusive box.  Rounds visit Y-, Y+, X-, X+, Z-, Z+; a face moves out by one voxel when it is not on
// the map's border and the slab one voxel beyond it, with the ranges the cube has AT THAT MOMENT, is free; the first round that
// moves nothing is the last.  The seed's own byte is never looked at.  Every round that goes on moves a face, so at most
// X + Y + Z rounds run whatever itr_inflate_max is.  Returns the number of table queries made.
template <class BoxFn>
DIRECT_CUBECOR_HD int inflate(const BoxFn& obstacles, int X, int Y, int Z, int sx, int sy, int sz, int itr_inflate_max, int* c) {
  int x0 = sx, x1 = sx, y0 = sy, y1 = sy, z0 = sz, z1 = sz, queries = 0;
  for (int it = 0; it < itr_inflate_max; it++) {
    bool moved = false;
    if (y0 > 0) {
      queries++;
      if (obstacles(x0, y0 - 1, z0, x1, y0 - 1, z1) == 0) { y0--; moved = true; }
    }
    if (y1 < Y - 1) {
      queries++;
      if (obstacles(x0, y1 + 1, z0, x1, y1 + 1, z1) == 0) { y1++; moved = true; }
    }
    if (x0 > 0) {
      queries++;
      if (obstacles(x0 - 1, y0, z0, x0 - 1, y1, z1) == 0) { x0--; moved = true; }
    }
    if (x1 < X - 1) {
      queries++;
      if (obstacles(x1 + 1, y0, z0, x1 + 1, y1, z1) == 0) { x1++; moved = true; }
    }
    if (z0 > 0) {
      queries++;
      if (obstacles(x0, y0, z0 - 1, x1, y1, z0 - 1) == 0) { z0--; moved = true; }
    }
    if (z1 < Z - 1) {
      queries++;
      if (obstacles(x0, y0, z1 + 1, x1, y1, z1 + 1) == 0) { z1++; moved = true; }
    }
    if (!moved) break;
  }
  c[0] = x0; c[1] = y0; c[2] = z0; c[3] = x1; c[4] = y1; c[5] = z1;
  return queries;
}

// ---- planes and centre of a cube: what direct_cluster_hull_planes_batch returns for the cube's resident cluster ------------------
// The cluster k_inflate leaves for a cube is its surface voxels in x, y, z order, and its lattice points (hull::lattice_point:
// voxel centres q = 2 index + 1, or the voxels' corners q +/- 1 when the cube is one voxel thick along an axis -
// checkDegeneratePoly) span a box.  The hull's facets are that box's six faces: primitive normals +/- e_a, ranked by
// hull::plane_cmp, converted by hull::plane_world.  The corners are the box's eight, in the order of their first appearance in
// the cluster: the voxel order (x, then y, then z) decides between corners of different voxels, which is the case along every
// axis the cube is thicker than one voxel; lattice_point's corner order (x, then y, then z again) decides inside a voxel, along
// the other axes.  The centre is step 4 of k_hull_finish: the mean, over the planes in rank order, of the first corner on each.
// planes[6][4], center[3]; returns the degenerate flag.
DIRECT_CUBECOR_HD int cube_polytope(const int* c, double res, const double* lower, double* planes, double* center) {
  DIRECT_CUBECOR_NO_CONTRACT
  const bool thick[3] = {c[0] != c[3], c[1] != c[4], c[2] != c[5]};
  const int degenerate = (thick[0] && thick[1] && thick[2]) ? 0 : 1;
  int qlo[3], qhi[3];
  hull::lattice_point(c[0], c[1], c[2], degenerate, 0, qlo[0], qlo[1], qlo[2]);
  hull::lattice_point(c[3], c[4], c[5], degenerate, 7, qhi[0], qhi[1], qhi[2]);
  hull::i64 P[kPlanes][4];
  int n = 0;
  for (int a = 0; a < 3; a++)
    for (int s = 0; s < 2; s++) {  // n . q + K <= 0 inside: -q_a + qlo_a <= 0 and q_a - qhi_a <= 0
      hull::i64 cand[4] = {0, 0, 0, s ? -(hull::i64)qhi[a] : (hull::i64)qlo[a]};
      cand[a] = s ? 1 : -1;
      int at = n++;
      for (; at > 0 && hull::plane_cmp(cand, P[at - 1]) < 0; at--)
        for (int k = 0; k < 4; k++) P[at][k] = P[at - 1][k];
      for (int k = 0; k < 4; k++) P[at][k] = cand[k];
    }
  for (int t = 0; t < kPlanes; t++) hull::plane_world(P[t], res, lower, degenerate, planes + 4 * t);
  int order[3], m = 0;  // the axes from the most to the least significant in the corners' order
  for (int a = 0; a < 3; a++)
    if (thick[a]) order[m++] = a;
  for (int a = 0; a < 3; a++)
    if (!thick[a]) order[m++] = a;
  double cs[3] = {0.0, 0.0, 0.0};
  for (int t = 0; t < kPlanes; t++)
    for (int r = 0; r < 8; r++) {
      int q[3];
      for (int j = 0; j < 3; j++) q[order[j]] = ((r >> (2 - j)) & 1) ? qhi[order[j]] : qlo[order[j]];
      if (P[t][0] * q[0] + P[t][1] * q[1] + P[t][2] * q[2] + P[t][3] != 0) continue;
      for (int a = 0; a < 3; a++) cs[a] = cs[a] + hull::world_coord(q[a], res, lower[a], degenerate);
      break;
    }
  for (int a = 0; a < 3; a++) center[a] = cs[a] / (double)kPlanes;
  return degenerate;
}

// ---- the walk: polyhedronGenerator::walk (direct_amd/host/poly_utils.hpp; global_planner/src/utils/poly_utils.cpp:391-449, 508-557)
// index2Coord (:20-29)
DIRECT_CUBECOR_HD void index2coord(const int32_t* idx, double res, const double* lower, double* cur) {
  DIRECT_CUBECOR_NO_CONTRACT
  for (int a = 0; a < 3; a++) cur[a] = idx[a] * res + 0.5 * res + lower[a];
}
// one plane's term of isOutsidePolytope (:42-52): in double, left to right.  Kept as the reference writes it: below a resolution
// of 0.02 the margin 0.01 admits a voxel centre one voxel outside the cube, and the host walk behaves that way.
DIRECT_CUBECOR_HD bool plane_excludes(const double* cur, const double* pl) {
  DIRECT_CUBECOR_NO_CONTRACT
  return cur[0] * pl[0] + cur[1] * pl[1] + cur[2] * pl[2] + pl[3] > 0.01;
}
DIRECT_CUBECOR_HD bool outside_polytope(const double* cur, const double* planes) {
  for (int t = 0; t < kPlanes; t++)
    if (plane_excludes(cur, planes + 4 * t)) return true;
  return false;
}

// The walk of one path from an empty corridor, stated serially (k_cube_walk runs it with one wave): path[len][3] voxel indices
// inside the map, cube[len][6] the cube of every one of them.  A point whose coordinates equal those of the point visited before
// it is skipped.  With pop_back (corridorGeneration, :524-528) a point inside the last-but-one polytope removes the last one.  A
// point for which the corridor is empty, or that lies outside the latest polytope, appends the cube of its own voxel.  stack[len]
// receives the path index of every polytope of the corridor; returns their number.
DIRECT_CUBECOR_HD int walk(const int32_t* path, int len, const int* cube, double res, const double* lower, int pop_back, int* stack) {
  int n = 0;
  double latest[4 * kPlanes] = {0.0}, prev[4 * kPlanes] = {0.0}, ctr[3];
  double lst[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  for (int i = 0; i < len; i++) {
    double cur[3];
    index2coord(path + 3 * i, res, lower, cur);
    if (cur[0] == lst[0] && cur[1] == lst[1] && cur[2] == lst[2]) continue;
    if (pop_back && n > 1 && !outside_polytope(cur, prev)) {
      n--;
      for (int k = 0; k < 4 * kPlanes; k++) latest[k] = prev[k];
      if (n > 1) cube_polytope(cube + 6 * stack[n - 2], res, lower, prev, ctr);
    }
    if (n == 0 || outside_polytope(cur, latest)) {
      for (int k = 0; k < 4 * kPlanes; k++) prev[k] = latest[k];
      cube_polytope(cube + 6 * i, res, lower, latest, ctr);
      stack[n++] = i;
    }
    for (int a = 0; a < 3; a++) lst[a] = cur[a];
  }
  return n;
}

}  // namespace cubecor
}  // namespace direct
