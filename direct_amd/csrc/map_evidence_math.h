// Arithmetic of direct_cluster_map_integrate_scan_evidence (include/direct_cluster.h, "occupancy evidence per voxel"): what one
// scan does to the evidence byte of one voxel, and when that byte means "occupied".  Integers only, plain C++ behind the
// qualifier macro of map_cloud_math.h: the kernels of map_evidence.h call these functions, and g++ compiles the same header for
// the CPU tests (tests/evidence_harness.py).  The walk and the dilation are map_scan_math.h's, unchanged.
//
// THE EVIDENCE GRID is one int8 per voxel in the map's layout, 0 = no information.  A scan first builds a TOUCH byte per voxel
// (0 not touched, 1 passed by a ray, 2 the voxel of a return; a return beats a pass), then folds it ONCE per voxel:
//   t == 2   e = min(e + hit, ev_max)
//   t == 1   e = max(e - miss, ev_min)
//   t == 0   e unchanged, even where it lies outside [ev_min, ev_max] (an earlier call with other limits, or set_evidence)
// in int arithmetic, and the voxel is occupied when e >= occ.  With one update per voxel and scan the result depends neither on
// the order of the points nor on the launch shape.  -128 is never stored: store_clamp keeps the range symmetric.
#pragma once
#include <stdint.h>

#include "map_cloud_math.h"

namespace direct {
namespace mapevid {

constexpr int kNone = 0, kPass = 1, kHit = 2;  // the touch byte
constexpr int kEvLimit = 127;                  // |evidence| never exceeds it

struct Params {
  int hit, miss;        // added for a return / subtracted for a pass, 1 .. 127 each
  int ev_min, ev_max;   // clamp of a TOUCHED voxel: -127 <= ev_min <= 0, occ <= ev_max <= 127
  int occ;              // occupied when e >= occ; 1 <= occ <= ev_max
};

// What a call with these parameters is refused with, or null; in the order hit, miss, ev_min, ev_max, occ, reserved
DIRECT_MAPCLOUD_HD const char* refusal(const Params& P, const int32_t* reserved /* [3] */) {
  if (P.hit < 1 || P.hit > kEvLimit) return "hit must lie in 1 .. 127";
  if (P.miss < 1 || P.miss > kEvLimit) return "miss must lie in 1 .. 127";
  if (P.ev_min < -kEvLimit || P.ev_min > 0) return "ev_min must lie in -127 .. 0";
  if (P.ev_max < 1 || P.ev_max > kEvLimit) return "ev_max must lie in 1 .. 127";
  if (P.occ < 1 || P.occ > P.ev_max) return "occ must lie in 1 .. ev_max";
  if (reserved[0] != 0 || reserved[1] != 0 || reserved[2] != 0) return "reserved must be 0";
  return nullptr;
}

// the evidence of a voxel after a scan that touched it as t
DIRECT_MAPCLOUD_HD int fold(int e, int t, const Params& P) {
  if (t == kHit) {
    const int s = e + P.hit;
    return s < P.ev_max ? s : P.ev_max;
  }
  if (t == kPass) {
    const int s = e - P.miss;
    return s > P.ev_min ? s : P.ev_min;
  }
  return e;
}
DIRECT_MAPCLOUD_HD bool occupied(int e, const Params& P) { return e >= P.occ; }
DIRECT_MAPCLOUD_HD int adopt(uint8_t map_byte, const Params& P) { return map_byte == 1 ? P.ev_max : 0; }  // DIRECT_SCAN_ADOPT
DIRECT_MAPCLOUD_HD int8_t store_clamp(int v) { return (int8_t)(v < -kEvLimit ? -kEvLimit : v); }          // set_evidence

}  // namespace mapevid
}  // namespace direct
