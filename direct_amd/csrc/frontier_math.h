// Rules of direct_cluster_frontier (include/direct_cluster.h, "frontier goals"): which voxels lie on the boundary between what the
// tracked scans have observed and what they have not, which of their components are kept, the centroid voxel of a component and
// the member that represents it.  Plain C++ behind a qualifier macro: the kernels of frontier.h call these functions, and g++
// compiles the same header for the CPU tests (tests/frontier_harness.py).  Integers only: there is nothing a compiler could
// contract.  There is no reference counterpart.
//
//   frontier voxel   known[v] != 0, and freecomp::enterable(map, d2, v, min_d2) - the graph of the path calls, so every frontier
//                    voxel is a legal goal of grid_paths_fan under the same floor - and at least one of the 6 face neighbours
//                    INSIDE the map has known == 0.  The outside of the map is not unknown space.
//   component        a 26-connected component of the frontier voxels, labelled by its smallest linear index.  The labelling is
//                    free_comp.h's, run on a MASK byte grid that is 0 exactly on frontier voxels: enterable(mask, null, v, 0) is
//                    then "v is a frontier voxel".
//   kept             size >= min_size; the kept components in ascending label order take the slots 0, 1, ...
//   centroid voxel   c_a = (2 * sum_a + n) / (2 * n) per axis in int64: the mean rounded half up.  It may be occupied, unknown or
//                    no member at all.
//   representative   the member that minimises ((min(dist2, 0xffffffff)) << 32) | linear index, dist2 = sum (v_a - c_a)^2 in
//                    int64: the member nearest the centroid voxel, ties to the smaller index by construction of the key.
// Sums and minima are order-independent integers: no output depends on the launch shape.
#pragma once
#include <stdint.h>

#include "free_comp_math.h"

namespace direct {
namespace frontier {

constexpr unsigned long long kNoKey = ~0ull;  // the minimum's neutral element: above every key of a member

// the mask byte of voxel v = (x, y, z): 0 on a frontier voxel, 1 elsewhere
DIRECT_FREECOMP_HD uint8_t mask_byte(const uint8_t* map, const uint8_t* known, const int32_t* d2, int x, int y, int z, int X, int Y, int Z,
                                     int32_t min_d2) {
  const long long v = ((long long)x * Y + y) * Z + z;
  if (known[v] == 0 || !freecomp::enterable(map, d2, v, min_d2)) return 1;
  const long long YZ = (long long)Y * Z;
  const bool unseen = (x > 0 && known[v - YZ] == 0) || (x < X - 1 && known[v + YZ] == 0) || (y > 0 && known[v - Z] == 0) ||
                      (y < Y - 1 && known[v + Z] == 0) || (z > 0 && known[v - 1] == 0) || (z < Z - 1 && known[v + 1] == 0);
  return unseen ? 0 : 1;
}

// v is the root of a kept component (label and size as free_comp.h leaves them)
DIRECT_FREECOMP_HD bool kept_root(int32_t label_v, int32_t size_v, long long v, int32_t min_size) {
  return label_v == (int32_t)v && size_v >= min_size;
}

// The coordinates of up to 64 voxels (each below 1024) summed in ONE 64-bit word: 21 bits per axis
DIRECT_FREECOMP_HD unsigned long long pack_xyz(int x, int y, int z) {
  return (unsigned long long)x | ((unsigned long long)y << 21) | ((unsigned long long)z << 42);
}
DIRECT_FREECOMP_HD long long packed_axis(unsigned long long s, int a) { return (long long)((s >> (21 * a)) & 0x1fffffull); }

DIRECT_FREECOMP_HD int32_t centroid_axis(long long sum, long long n) { return (int32_t)((2 * sum + n) / (2 * n)); }

DIRECT_FREECOMP_HD unsigned long long rep_key(int x, int y, int z, const int32_t* c, long long v) {
  const long long dx = x - c[0], dy = y - c[1], dz = z - c[2];
  const long long dist2 = dx * dx + dy * dy + dz * dz;
  const unsigned long long hi = dist2 > 0xffffffffll ? 0xffffffffull : (unsigned long long)dist2;
  return (hi << 32) | (unsigned long long)(uint32_t)v;
}
DIRECT_FREECOMP_HD int32_t key_voxel(unsigned long long key) { return (int32_t)(key & 0xffffffffull); }

}  // namespace frontier
}  // namespace direct
