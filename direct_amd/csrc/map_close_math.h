// Arithmetic of the unknown policy of the cluster handle (include/direct_cluster.h, "unknown space as occupied"): what the map byte
// of one voxel is when unobserved space is closed, how the close pass groups the voxels, and what the policy refuses.  Integers
// only, plain C++ behind the qualifier macro of map_cloud_math.h: k_scan_close of map_close.h calls these functions, and g++
// compiles the same header for the CPU tests (tests/unknown_policy_harness.py).
//
// Under DIRECT_UNKNOWN_OCCUPIED a scan derives TWO grids from the scan grid `raw` and the known grid:
//   open[v] = dilate(raw, inflate)[v]        what the scan produces under DIRECT_UNKNOWN_FREE, byte for byte
//   map[v]  = open[v] | (known[v] == 0)      unknown space is closed and NOT inflated
// A known voxel is occupied in the map exactly when it is occupied in the open map; both are per-voxel functions of grids that
// depend neither on the order of the points nor on the launch shape.
#pragma once
#include <stdint.h>

#include "map_cloud_math.h"

namespace direct {
namespace mapclose {

constexpr int kFree = 0, kOccupied = 1;  // DIRECT_UNKNOWN_FREE, DIRECT_UNKNOWN_OCCUPIED
constexpr int kGroup = 16;               // voxels per lane and trip of the close pass: one 128-bit word per grid
constexpr int kTrackKnown = 1;           // DIRECT_SCAN_TRACK_KNOWN

DIRECT_MAPCLOUD_HD bool policy_known(int32_t policy) { return policy == kFree || policy == kOccupied; }

// What a scan with these flags is refused with under this policy, or null: the known grid of an untracked scan is dropped, and
// a map closed by no known grid would be all ones
DIRECT_MAPCLOUD_HD const char* scan_refusal(int32_t policy, int32_t flags) {
  if (policy == kOccupied && (flags & kTrackKnown) == 0) return "DIRECT_UNKNOWN_OCCUPIED: the scan must set DIRECT_SCAN_TRACK_KNOWN";
  return nullptr;
}

// the byte rule; open is 0 or 1 (the dilation writes nothing else)
DIRECT_MAPCLOUD_HD uint8_t close_byte(uint8_t open, uint8_t known) { return (uint8_t)((open != 0) | (known == 0)); }
// closed by the policy alone: occupied in the map, free in the open map
DIRECT_MAPCLOUD_HD bool closed(uint8_t open, uint8_t map) { return map == 1 && open == 0; }

// groups of kGroup voxels in a grid of G; all but the last hold kGroup, the last G - 16 * (groups - 1) in 1 .. 16
DIRECT_MAPCLOUD_HD long long groups(long long G) { return (G + kGroup - 1) / kGroup; }
DIRECT_MAPCLOUD_HD long long group_at(long long g) { return g * kGroup; }
DIRECT_MAPCLOUD_HD int group_size(long long G, long long g) {
  const long long left = G - group_at(g);
  return left < kGroup ? (int)left : kGroup;
}

}  // namespace mapclose
}  // namespace direct
