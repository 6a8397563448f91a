// Arithmetic of direct_cluster_cube_corridor_clear_batch (include/direct_cluster.h, "radius-aware cube corridors"): the predicate
// "below the floor", the index arithmetic of the floor table, and the choice of the cache slot a call uses.  Everything else - the
// cube, its planes, the walk - is cube_corridor_math.h.  Plain C++ behind a qualifier macro: k_floor_fill of
// cube_corridor_clear.h and the host code of direct_cluster.hip call these functions, and g++ compiles the same header for the
// CPU tests (tests/cube_corridor_clear_harness.py).  All integer.
//
// THE FLOOR TABLE is a summed-area table with the layout and strides of Dev::sat: (X + 1)(Y + 1)(Z + 1) int entries, entry
// (x, y, z) at x * sat_yz + y * sat_z + z with sat_z = Z + 1 and sat_yz = (Y + 1) * sat_z, holding the number of voxels below the
// floor in [0, x) x [0, y) x [0, z).  Before the three running sums, entry (x, y, z) is 1 when x, y, z > 0 and voxel
// (x - 1, y - 1, z - 1) is below the floor, else 0: the plane x == 0, y == 0 or z == 0 is the zero border.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DIRECT_CUBECLEAR_HD __host__ __device__ __forceinline__
#else
#define DIRECT_CUBECLEAR_HD inline
#endif

namespace direct {
namespace cubecor {

constexpr int kFloorSlots = 2;  // floor tables resident on a handle: two vehicle sizes on one map never rebuild

// min_d2 <= 1 is the map's own table: D2 is 0 exactly on bytes == 1, so "below the floor" is "occupied" (the neutral rule of
// grid_path_clear_math.h)
DIRECT_CUBECLEAR_HD bool floor_neutral(int32_t min_d2) { return min_d2 <= 1; }

// a voxel of stored field value d2 counts as an obstacle of the cube
DIRECT_CUBECLEAR_HD bool below_floor(int32_t d2, int32_t min_d2) { return d2 < min_d2; }

// Entry i of the table of an X x Y x Z map, i < (X + 1) * sat_yz: -1 on the zero border, else the index of the voxel
// (x - 1, y - 1, z - 1) in the field (z fastest: entries adjacent in z are voxels adjacent in the field)
DIRECT_CUBECLEAR_HD int floor_entry_voxel(int i, int Y, int Z) {
  const int sat_z = Z + 1, sat_yz = (Y + 1) * sat_z;
  const int x = i / sat_yz, r = i - x * sat_yz, y = r / sat_z, z = r - y * sat_z;
  if (x == 0 || y == 0 || z == 0) return -1;
  return ((x - 1) * Y + (y - 1)) * Z + (z - 1);
}

// the 0 / 1 value of entry i before the running sums
DIRECT_CUBECLEAR_HD int floor_entry(const int32_t* d2, int i, int Y, int Z, int32_t min_d2) {
  const int v = floor_entry_voxel(i, Y, Z);
  return v >= 0 && below_floor(d2[v], min_d2) ? 1 : 0;
}

// ---- the cache of floor tables ---------------------------------------------------------------------------------------------
// A slot holds the table of one (min_d2, field serial); the serial counts the successful builds of the distance field, so a
// table of an earlier field never matches.  `used` is the value of the caller's clock at the slot's last use.
struct FloorSlot {
  int32_t min_d2;
  int valid;                  // 0: empty (never built, or its build failed)
  unsigned long long serial;  // the field it was built from
  unsigned long long used;
  long long count;            // voxels below the floor: the table's last entry
};

// The slot a clear-mode call uses: the valid slot of (min_d2, serial) if there is one (*hit = 1, nothing to build), else the
// victim a build goes into (*hit = 0): the first empty slot, or without one the least recently used.  n >= 1.
DIRECT_CUBECLEAR_HD int floor_slot_choose(const FloorSlot* s, int n, int32_t min_d2, unsigned long long serial, int* hit) {
  for (int k = 0; k < n; k++)
    if (s[k].valid && s[k].min_d2 == min_d2 && s[k].serial == serial) {
      *hit = 1;
      return k;
    }
  *hit = 0;
  int victim = 0;
  for (int k = 0; k < n; k++) {
    if (!s[k].valid) return k;
    if (s[k].used < s[victim].used) victim = k;
  }
  return victim;
}

}  // namespace cubecor
}  // namespace direct
