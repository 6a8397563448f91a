// Rules of direct_cluster_corridor_batch (include/direct_cluster.h, "cluster corridors"): the walk of polyhedronGenerator::walk
// (direct_amd/host/poly_utils.hpp; global_planner/src/utils/poly_utils.cpp:391-449, 508-557) for a batch of grid paths, in the
// reference's is_cluster_on == true mode, cut into ROUNDS: a row walks until it needs a polytope, the seeds that are due in a
// round are de-duplicated by voxel, generated in chunks, and handed back to every row that waits for them.  Plain C++ behind the
// qualifier macro of cube_corridor_math.h: the kernels of cluster_corridor.h call these functions with a wave-wide plane test, and
// g++ compiles the same header for the CPU tests (tests/cluster_corridor_harness.py) with a serial one.
//
// A polytope is a function of its seed voxel and the map alone (getConvexPoly), so sharing one generation among the rows that ask
// for the same voxel in the same round changes no byte of any row.  The plane test is cube_corridor_math.h's plane_excludes on the
// DOUBLE planes of the row's stack, whatever type the outputs have.
#pragma once
#include "cube_corridor_math.h"

namespace direct {
namespace clucor {

// per-row codes: DIRECT_CORRIDOR_*
constexpr int kOk = 0, kOverflow = 1, kBadPath = 2, kNoPolytope = 3, kTooManyPlanes = 4;
// Row::state
constexpr int kWalking = 0, kDue = 1, kDone = 2;
constexpr int kNoOwner = 0x7f7f7f7f;  // an entry of the per-voxel owner table that no row has touched (a 0x7f byte fill; above any row index)
constexpr int kMinPlanes = 6;
constexpr int kHullOk = 0, kHullOverflow = 1;  // DIRECT_HULL_OK, DIRECT_HULL_OVERFLOW

// The walk state of one row.  `depth` polytopes lie on the row's plane stack; `last` is the voxel of the point visited before
// `next` (the reference keeps its coordinate: index2coord of it is that coordinate, bit for bit); in state kDue the row waits for
// the polytope of voxel `seed`, which the round's de-duplication filed under `slot` of the seed list.
struct Row {
  int32_t next, depth, code, state, slot, has_last, pops, pad;
  int32_t last[3], seed[3], pad2[2];
};

DIRECT_CUBECOR_HD bool voxel_inside(const int32_t* v, int X, int Y, int Z) {
  return v[0] >= 0 && v[0] < X && v[1] >= 0 && v[1] < Y && v[2] >= 0 && v[2] < Z;
}
DIRECT_CUBECOR_HD int voxel_index(const int32_t* v, int Y, int Z) { return (v[0] * Y + v[1]) * Z + v[2]; }

DIRECT_CUBECOR_HD Row row_start(bool bad_path) {
  Row r = {};
  r.code = bad_path ? kBadPath : kOk;
  r.state = bad_path ? kDone : kWalking;
  return r;
}

// One row until it is due or done.  outside(level, cur): does a plane of polytope `level` of the row's stack exclude cur.  Per
// point, in the reference's order: skip a point equal to the one visited before it; with pop_back, pop when the point is not
// outside the last-but-one polytope (:524-528) - the pop stands even when the row then has to wait or ends; a polytope is due
// when the corridor is empty or the point is outside the latest one.  A due point is NOT consumed: append() steps past it.  The
// loop ends after at most len - next + 1 trips.
template <class Outside>
DIRECT_CUBECOR_HD void advance(Row& r, const int32_t* path, int len, int seg_cap, int pop_back, double res, const double* lower,
                               const Outside& outside) {
  while (r.state == kWalking) {
    if (r.next >= len) {
      r.state = kDone;
      break;
    }
    const int32_t* v = path + 3 * r.next;
    double cur[3];
    cubecor::index2coord(v, res, lower, cur);
    if (r.has_last) {
      double lst[3];
      cubecor::index2coord(r.last, res, lower, lst);
      if (cur[0] == lst[0] && cur[1] == lst[1] && cur[2] == lst[2]) {
        r.next++;
        continue;
      }
    }
    if (pop_back && r.depth > 1 && !outside(r.depth - 2, cur)) {
      r.depth--;
      r.pops++;
    }
    if (r.depth == 0 || outside(r.depth - 1, cur)) {
      if (r.depth >= seg_cap) {  // polytope seg_cap + 1: the stack as it is now is what the row returns
        r.code = kOverflow;
        r.state = kDone;
        break;
      }
      for (int a = 0; a < 3; a++) r.seed[a] = v[a];
      r.state = kDue;
      break;
    }
    for (int a = 0; a < 3; a++) r.last[a] = v[a];
    r.has_last = 1;
    r.next++;
  }
}

// What a due row makes of its seed's generation: kOk (the caller then puts the polytope on level r.depth and calls push), or the
// code the row ends with.  gen_ok: the generation ended DIRECT_CLUSTER_OK.  The hull ran with a plane capacity of p_max, so a
// polytope with more facets comes back DIRECT_HULL_OVERFLOW with its true count.
DIRECT_CUBECOR_HD int judge(bool gen_ok, int hull_rtn, int n_planes, int p_max) {
  if (gen_ok && hull_rtn == kHullOverflow && n_planes > p_max) return kTooManyPlanes;
  if (!gen_ok || hull_rtn != kHullOk) return kNoPolytope;  // the reference's cdd-error branch (:548-552)
  return kOk;
}
DIRECT_CUBECOR_HD void stop(Row& r, int code) {
  r.code = code;
  r.state = kDone;
}
DIRECT_CUBECOR_HD void push(Row& r) {  // the polytope is on the stack: step past the point
  r.depth++;
  for (int a = 0; a < 3; a++) r.last[a] = r.seed[a];
  r.has_last = 1;
  r.next++;
  r.state = kWalking;
}

// The round's de-duplication, stated serially (k_corr_unique runs the same four steps with one workgroup): the owner of a voxel
// is the SMALLEST due row that asks for it; owners, in row order, fill seed_list[unique][3] and take slots 0, 1, ...; every due
// row gets its owner's slot; the touched table entries go back to kNoOwner.  table[X*Y*Z] must be all kNoOwner and is left so.
// Returns the number of unique seeds; *due receives the number of due rows.
inline int unique_seeds(Row* rows, int batch, int Y, int Z, int* table, int32_t* seed_list, int* due) {
  int n_due = 0, n_unique = 0;
  for (int b = 0; b < batch; b++)
    if (rows[b].state == kDue) {
      int& t = table[voxel_index(rows[b].seed, Y, Z)];
      t = b < t ? b : t;
      n_due++;
    }
  for (int b = 0; b < batch; b++)
    if (rows[b].state == kDue && table[voxel_index(rows[b].seed, Y, Z)] == b) {
      for (int a = 0; a < 3; a++) seed_list[3 * n_unique + a] = rows[b].seed[a];
      rows[b].slot = n_unique++;
    }
  for (int b = 0; b < batch; b++)
    if (rows[b].state == kDue) rows[b].slot = rows[table[voxel_index(rows[b].seed, Y, Z)]].slot;
  for (int b = 0; b < batch; b++)
    if (rows[b].state == kDue) table[voxel_index(rows[b].seed, Y, Z)] = kNoOwner;
  *due = n_due;
  return n_unique;
}

// Entry q of a row's planes output, [seg_cap][p_max][4] flattened: the stack's value inside the corridor and inside a polytope's
// planes, zero behind either.  st_planes / st_np are the row's slices of the stack.
DIRECT_CUBECOR_HD double emit_plane(const Row& r, const double* st_planes, const int32_t* st_np, int p_max, int q) {
  const int k = q / (4 * p_max), t = (q - k * 4 * p_max) / 4;
  return (k < r.depth && t < st_np[k]) ? st_planes[q] : 0.0;
}

}  // namespace clucor
}  // namespace direct
