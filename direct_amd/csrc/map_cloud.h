// Kernel of direct_cluster_map_from_cloud (include/direct_cluster.h, "the map from a point cloud"); included by
// direct_cluster.hip inside its anonymous namespace.  The arithmetic is map_cloud_math.h's, shared with the CPU tests.
//
// The voxels of one point are the Cartesian product of three per-axis index lists of at most 2s+1, 2s+1 and 2s_z+1 entries
// (the index along an axis depends on that axis' coordinate and offset alone), and z is the contiguous axis of the map.  A lane
// owns one (point, x-offset, y-offset): it computes its x and its y index once and walks the z list, writing the byte 1 into its
// column.  The z list is recomputed per entry and every entry is written on its own, so a list that clamping shortened, or that
// rounding left with a gap or a repeat, needs no special case.  Every writer of a voxel writes the same byte: no atomics, and the
// map does not depend on the order of the points or on the launch shape.  Neighbouring lanes (y-offset fastest) hit neighbouring
// columns, max_z bytes apart; lanes of different points scatter.  The whole map of the launch file (333 x 333 x 33 = 3.7 MB) fits
// in an XCD's 4 MB L2 and many times in the Infinity Cache, which absorb the scatter.  The points are NOT bucketed by x-slab first:
// on a cloud already sorted by x (what such a pass would hand the kernel, at no cost) the call is at most 0.09 ms of 1.17 ms faster
// and in places slower (tools/map_cloud_bench.py, profiles/map_cloud_bench.json) - less than any sort of 10^6
// points costs.
#pragma once
#include "map_cloud_math.h"

namespace mc = direct::mapcloud;

struct CloudDev {
  double lower[3], upper[3];
  double resolution, inv;
  int size[3];             // voxels per axis
  int s, sz, border, stride;
  long long n;             // points
  const float* xyz;        // [n][stride]
  uint8_t* map;            // [size[0] * size[1] * size[2]]
  unsigned long long* cnt; // [2] points skipped as non-finite, (point, offset) triples dropped
};

__global__ __launch_bounds__(256) void k_cloud_raster(CloudDev C) {
  const long long w = 2 * C.s + 1, ww = w * w, total = C.n * ww;
  const int nz = 2 * C.sz + 1;
  unsigned long long skipped = 0, dropped = 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long p = t / ww;
    const int r = (int)(t - p * ww), kx = r / (int)w - C.s, ky = r % (int)w - C.s;
    const float* q = C.xyz + p * C.stride;
    const float fx = q[0], fy = q[1], fz = q[2];
    if (!mc::is_finite3(fx, fy, fz)) {
      skipped += r == 0;
      continue;
    }
    const int ix = mc::axis_index(C.border, mc::shifted(fx, kx, C.resolution), C.lower[0], C.upper[0], C.inv, C.size[0]);
    const int iy = mc::axis_index(C.border, mc::shifted(fy, ky, C.resolution), C.lower[1], C.upper[1], C.inv, C.size[1]);
    if (ix < 0 || iy < 0) {
      dropped += nz;
      continue;
    }
    uint8_t* col = C.map + ((size_t)ix * C.size[1] + iy) * C.size[2];
    for (int kz = -C.sz; kz <= C.sz; kz++) {
      const int iz = mc::axis_index(C.border, mc::shifted(fz, kz, C.resolution), C.lower[2], C.upper[2], C.inv, C.size[2]);
      if (iz < 0) dropped++;
      else col[iz] = 1;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    skipped += __shfl_down(skipped, o);
    dropped += __shfl_down(dropped, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (skipped) atomicAdd(&C.cnt[0], skipped);
    if (dropped) atomicAdd(&C.cnt[1], dropped);
  }
}
