// Kernel of direct_cluster_cube_corridor_clear_batch (include/direct_cluster.h, "radius-aware cube corridors"): the floor table,
// the summed-area table of "stored D2 below min_d2" in the layout of Dev::sat.  Included from direct_cluster.hip inside its
// anonymous namespace, after Dev and k_sat_scan; the arithmetic is cube_corridor_clear_math.h (plain C++, also compiled by g++
// for tests/cube_corridor_clear_harness.py).
//
//   k_floor_fill  the 0 / 1 entries with the zero border, one lane per entry, striding over the table
// The three running sums are k_sat_scan on a Dev whose `sat` is the floor table, and the cubes and the walk are k_cube_inflate and
// k_cube_walk of cube_corridor.h given that Dev: box_obstacles then counts voxels below the floor.  No LDS, no atomics, and the
// one loop is bounded by the table's size.
#pragma once

// Adjacent lanes hold adjacent entries, which are adjacent in z (the fastest axis of table and field alike): a wave's loads from
// the field and its stores to the table are each contiguous but for the one-entry border at the end of every z line.  The table
// has fewer than 2^30 entries (direct_cluster_create) and the grid at most 2^18 lanes: the int index cannot overflow.
__global__ __launch_bounds__(256) void k_floor_fill(Dev D, const int32_t* d2, int32_t min_d2) {
  const int n = (D.max_x + 1) * D.sat_yz;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    D.sat[i] = cc::floor_entry(d2, i, D.max_y, D.max_z, min_d2);
}
