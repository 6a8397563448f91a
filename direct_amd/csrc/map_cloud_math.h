// Arithmetic of direct_cluster_map_from_cloud (include/direct_cluster.h, "the map from a point cloud"): how many voxel steps a
// cloud is inflated by, the coordinate of a point shifted by k steps, and the voxel index of a coordinate along one axis under
// the two border conventions.  Plain C++ behind a qualifier macro: the kernel of map_cloud.h calls these functions, and g++
// compiles the same header for the CPU tests (tests/map_cloud_harness.py).
//
// What is restated is rcvPointCloudCallBack (global_planner/src/teach_repeat_planner.cpp:523-581, "TRP"): every point of the
// cloud is shifted by every offset (x, y, z) of a (2s+1)^2 x (2s_z+1) box of voxel STEPS (:542-550), the shifted COORDINATE is
// quantised, and the voxel is marked.  Inflation therefore acts on coordinates and not on voxels: a float32 point that sits on a
// voxel face can round into either neighbour after the shift, and "the point's voxel, dilated by a box" is a different map.
//   s   = (int)round(cloud_margin * inv_resolution), inv_resolution = 1.0 / resolution computed once (TRP:537, 1201)
//   s_z = max(1, s / 2) in integer division (TRP:538): a margin of 0 still inflates by one voxel up and down in z
// The reference keeps two maps that disagree at the border:
//   clamp  the polytope generator's map gets setObs(coord2gridIndex(coord)) (TRP:553, 557; utils/a_star.h:141-149): the index is
//          min(max(int(q), 0), size - 1), a coordinate outside the map marks a border voxel
//   drop   the path finder's map gets setObs(x, y, z) (TRP:556; utils/a_star.cpp:74-85): a coordinate outside [lower, upper)
//          along any axis is discarded
// with q = (coord - lower) * inv_resolution in double.
//
// Defined HERE because the reference leaves it undefined:
//   * int(double) of a NaN or of a value outside int's range is undefined behaviour.  axis_index_clamp compares q against the
//     range first and never converts such a value; a point with a non-finite coordinate contributes nothing at all (is_finite3).
//   * In the path finder's setObs a coordinate in [size * resolution + lower, upper) passes the range test and indexes one past
//     the array (49.95 .. 50 at the launch file's values, where upper - lower is no multiple of the resolution).
//     axis_index_drop DROPS it: an index >= size is treated like a coordinate >= upper.
//
// Contraction: the shifted coordinate is (double)p + (double)k * resolution with BOTH roundings, as the reference's x86-64 build
// computes it; a fused multiply-add would round once and move points that sit on voxel faces.  This header switches contraction
// off itself, per function, with "#pragma clang fp contract(off)" where the compiler is clang (hipcc's default is to contract);
// under g++, which has no such pragma, the harness passes -ffp-contract=off.  The other expression, (coord - lower) * inv, is a
// difference that is multiplied: no multiply-add can be formed from it.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DIRECT_MAPCLOUD_HD __host__ __device__ __forceinline__
#else
#define DIRECT_MAPCLOUD_HD inline
#endif
#if defined(__clang__)
#define DIRECT_MAPCLOUD_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DIRECT_MAPCLOUD_NO_CONTRACT
#endif

namespace direct {
namespace mapcloud {

constexpr int kMaxSteps = 1024;  // the library refuses a larger s (maps have at most 1024 voxels per axis)

// TRP:537-538.  The caller has checked that cloud_margin * inv is finite, not negative and within int's range.
DIRECT_MAPCLOUD_HD void inf_steps(double cloud_margin, double resolution, int* s, int* sz) {
  const double inv = 1.0 / resolution;
  *s = (int)round(cloud_margin * inv);
  *sz = *s / 2 > 1 ? *s / 2 : 1;
}

DIRECT_MAPCLOUD_HD bool is_finite3(float x, float y, float z) {
  // x - x is 0 for a finite x and NaN for +/-inf and NaN
  return (x - x) == 0.0f && (y - y) == 0.0f && (z - z) == 0.0f;
}

// TRP:548-550: pt.x + x * _resolution with pt.x a float, x an int, _resolution a double
DIRECT_MAPCLOUD_HD double shifted(float p, int k, double resolution) {
  DIRECT_MAPCLOUD_NO_CONTRACT
  const double step = (double)k * resolution;
  return (double)p + step;
}

// coord2gridIndex along one axis (a_star.h:141-149).  Equals min(max(int(q), 0), size - 1) wherever that is defined: int(q) is 0
// for every q in (-1, 1) and negative below, so "q < 1" is the lower clamp.  A NaN q (non-finite lower) gives 0.
DIRECT_MAPCLOUD_HD int axis_index_clamp(double coord, double lower, double inv, int size) {
  DIRECT_MAPCLOUD_NO_CONTRACT
  const double q = (coord - lower) * inv;
  if (q >= (double)size) return size - 1;
  if (!(q >= 1.0)) return 0;
  return (int)q;
}

// setObs(x, y, z) along one axis (a_star.cpp:74-85): -1 is "dropped".  coord >= lower makes q >= 0, and q >= size is exactly
// "(int)q >= size" then: the case in which the reference writes past its array, dropped here.
DIRECT_MAPCLOUD_HD int axis_index_drop(double coord, double lower, double upper, double inv, int size) {
  DIRECT_MAPCLOUD_NO_CONTRACT
  if (!(coord >= lower) || !(coord < upper)) return -1;
  const double q = (coord - lower) * inv;
  if (!(q < (double)size)) return -1;
  return (int)q;
}

constexpr int kBorderClamp = 0, kBorderDrop = 1;  // DIRECT_MAP_BORDER_CLAMP / DIRECT_MAP_BORDER_DROP

DIRECT_MAPCLOUD_HD int axis_index(int border, double coord, double lower, double upper, double inv, int size) {
  return border == kBorderDrop ? axis_index_drop(coord, lower, upper, inv, size) : axis_index_clamp(coord, lower, inv, size);
}

}  // namespace mapcloud
}  // namespace direct
