// Arithmetic of direct_cluster_grid_path_fan_batch (include/direct_cluster.h, "shared-start grid paths"): which goals of a source
// count for its pruning bound, and the fold that makes the bound.  Everything else - the graph, the two costs, the relaxation,
// the acceptance rule, the wake mask, the predecessor rules - is grid_path_math.h and grid_path_clear_math.h, which this header
// includes.  Plain C++ behind the same qualifier macro: the kernels of grid_path_fan.h call these functions, and g++ compiles the
// same header for the CPU tests (tests/grid_path_fan_harness.py).  No floating-point operation is added: the bound is a maximum
// of stored doubles, which no order of evaluation can change.
#pragma once
#include "grid_path_clear_math.h"

namespace direct {
namespace gridpath {

// A goal INSIDE the map, of a source inside the map, is eligible when it is the source itself or a voxel a move may enter (byte
// 0 and stored D2 >= min_d2; the plain cost passes d2 = 0, min_d2 = 0).  Only eligible goals can ever hold a finite value, so
// only they may keep the bound up: a goal that is NO_PATH before anything runs (occupied, or below the floor) stays +inf for
// ever and would switch the pruning off for its whole group.
DIRECT_GRIDPATH_HD bool fan_eligible(bool is_source, uint8_t byte, int32_t d2, int32_t min_d2) {
  return is_source || clear_open(byte, d2, min_d2);
}

// bound(s) = max over the eligible goals of d_s(goal), 0.0 without one (then nothing is relaxed: accept() refuses every
// candidate, all of which are >= 1).  Values are never NaN, so the maximum does not depend on the order of the fold.
DIRECT_GRIDPATH_HD double fan_bound_fold(double acc, double v) { return v > acc ? v : acc; }

// rounds between two refreshes of the bound on the device: 1 (before every round) or kFanRoundsPerCheck (once per batch of
// enqueued rounds).  The bound only falls, so a value read late is still valid; both settings end on the same bytes.
constexpr int kFanRoundsPerCheck = 8;

}  // namespace gridpath
}  // namespace direct
