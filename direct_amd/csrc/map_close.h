// Kernel of the unknown policy DIRECT_UNKNOWN_OCCUPIED (include/direct_cluster.h, "unknown space as occupied"); included by
// direct_cluster.hip inside its anonymous namespace, behind map_evidence.h, whose 16-byte group moves it reuses.  The byte rule
// and the group arithmetic are map_close_math.h's, shared with the CPU tests.
//
// Under the policy the last (x) pass of k_scan_dilate runs in its non-counting form into the resident OPEN MAP, and
//   k_scan_close   takes over that pass's role for the map: one pass over the grid, a lane owns 16 consecutive voxels and moves
//                  open map, known grid, scan grid and the map's previous bytes as one 128-bit word each.  map = open |
//                  (known == 0); a group of the map is stored only when it changed, so a scan that teaches nothing writes
//                  nothing.  The last group of a grid whose voxel count is no multiple of 16 goes byte by byte and never reads
//                  past the end.  It counts what the last dilation pass counts (ones of the scan grid, ones of the map, voxels
//                  of the map set and cleared) into the scan's counters, and `closed` (map 1, open 0) and the open map's ones
//                  into two counters of its own.
// The loop is a grid-stride loop bounded by kScanMaxBlocks workgroups; no LDS, no waiting between waves.  Counters go through
// scan_count.  Traffic: four bytes read per voxel and at most one written, as k_evid_fold with the known grid.
#pragma once
#include "map_close_math.h"
#include "map_evidence.h"

namespace mcl = direct::mapclose;

static_assert(mcl::kGroup == kEvidGroup, "the close pass moves the fold's groups");
enum { kCloseClosed = 0, kCloseOpenOnes, kCloseCounters };

struct CloseDev {
  long long G;                // voxels
  const uint8_t* open;        // [G] the open map: the dilated scan grid, 0 or 1
  const uint8_t* known;       // [G] the known grid
  const uint8_t* raw;         // [G] the scan grid, whose ones are counted
  uint8_t* map;               // [G] the map: read as the bytes "before", written where they differ
  unsigned long long* cnt;    // [kScanCounters] the scan's counters
  unsigned long long* more;   // [kCloseCounters]
};

__global__ __launch_bounds__(256) void k_scan_close(CloseDev C) {
  // per lane in 32 bits: a lane sees G / (kScanMaxBlocks * 256) voxels at most, widened once behind the loop
  unsigned int raw_ones = 0, map_ones = 0, set = 0, cleared = 0, closed = 0, open_ones = 0;
  const long long groups = mcl::groups(C.G);
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long at = mcl::group_at(g);
    const int n = mcl::group_size(C.G, g);
    const Evid16 o = evid_load(C.open + at, n);
    const Evid16 kn = evid_load(C.known + at, n);
    const Evid16 r = evid_load(C.raw + at, n);
    const Evid16 m0 = evid_load(C.map + at, n);
    Evid16 m1 = {{0u, 0u, 0u, 0u}};
#pragma unroll
    for (int k = 0; k < kEvidGroup; k++) {
      const int w = k >> 2, sh = 8 * (k & 3);
      const uint8_t ob = (uint8_t)(o.w[w] >> sh), kb = (uint8_t)(kn.w[w] >> sh), rb = (uint8_t)(r.w[w] >> sh);
      const uint8_t before = (uint8_t)(m0.w[w] >> sh);
      const bool live = k < n;  // the bytes behind the end of the tail are zero in every word and stay so
      const uint8_t now = live ? mcl::close_byte(ob, kb) : (uint8_t)0;
      m1.w[w] |= (uint32_t)now << sh;
      raw_ones += live && rb == 1;
      map_ones += now;
      set += live && before != now && now == 1;
      cleared += live && before != now && now == 0;
      closed += live && mcl::closed(ob, now);
      open_ones += live && ob == 1;
    }
    if (evid_differ(m0, m1)) evid_store(C.map + at, n, m1);
  }
  scan_count(raw_ones, &C.cnt[kScanRawOnes]);
  scan_count(map_ones, &C.cnt[kScanMapOnes]);
  scan_count(set, &C.cnt[kScanSet]);
  scan_count(cleared, &C.cnt[kScanCleared]);
  scan_count(closed, &C.more[kCloseClosed]);
  scan_count(open_ones, &C.more[kCloseOpenOnes]);
}
