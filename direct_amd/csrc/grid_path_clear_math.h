// Arithmetic of direct_cluster_grid_path_clear_batch (include/direct_cluster.h, "clearance-aware grid paths"): the graph with a
// floor on the distance field, the penalty of an entered voxel, the relaxation of one voxel with that penalty, and the
// predecessor rule of the read-back.  Everything else - the tile, the weights, the acceptance rule with the pruning bound, the
// wake mask - is grid_path_math.h, which this header includes.  Plain C++ behind the same qualifier macro: the kernels of
// grid_path_clear.h call these functions, and g++ compiles the same header for the CPU tests (tests/grid_path_clear_harness.py).
// The floating-point operations are two double additions per move, step weight first, then the entered voxel's penalty: nothing
// a compiler could contract, and contraction is switched off all the same (clang: the pragma below; g++: -ffp-contract=off from
// the harness), so the two compilers produce the same bits.
//
//   d(v) = fl( min_u fl(d(u) + w(u, v)) + pen(v) )
// pen(v) does not depend on u and a -> fl(a + p) is monotone, so min_u fl(fl(d(u) + w) + pen(v)) is the same double: the
// minimum is taken BEFORE the second addition, one addition per sweep and voxel instead of 26.
#pragma once
#include "grid_path_math.h"

#if defined(__clang__)
#define DIRECT_GRIDPATH_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DIRECT_GRIDPATH_NO_CONTRACT
#endif

namespace direct {
namespace gridpath {

constexpr int kMaxPenalty = 65536;  // entries of the penalty table at most (D2 below 256^2)

// A move goes INTO a voxel inside the map whose byte is 0 and whose stored D2 is at least min_d2.  D2 is 0 exactly on occupied
// voxels, so min_d2 <= 1 is the graph of grid_path_math.h.
DIRECT_GRIDPATH_HD bool clear_open(uint8_t byte, int32_t d2, int32_t min_d2) { return byte == 0 && d2 >= min_d2; }

// pen(v) = penalty[D2[v]] below n_penalty, else 0.0 (penalty may be null when n_penalty is 0).  A stored D2 is never negative;
// the unsigned comparison keeps the index inside the table whatever the field holds.
DIRECT_GRIDPATH_HD double clear_penalty(const double* penalty, int32_t n_penalty, int32_t d2) {
  return (uint32_t)d2 < (uint32_t)n_penalty ? penalty[d2] : 0.0;
}

// the candidate of the voxel staged at index c: the minimum of grid_path_math.h's relaxation, then the voxel's own penalty
DIRECT_GRIDPATH_HD double clear_candidate(const double* staged, int c, double pen) {
  DIRECT_GRIDPATH_NO_CONTRACT
  const double best = relax_candidate(staged, c);
  return best + pen;
}

// Read-back: neighbour k (value du, +inf when it is outside the map) is a predecessor of a voxel of value dv and penalty pen
// when the two additions the relaxation made reproduce dv to the bit.  The path takes the lowest such k.
DIRECT_GRIDPATH_HD bool clear_is_predecessor(double du, int k, double pen, double dv) {
  DIRECT_GRIDPATH_NO_CONTRACT
  const double a = du + weight_of(k);
  return a + pen == dv;
}

}  // namespace gridpath
}  // namespace direct
