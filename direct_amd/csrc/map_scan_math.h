// Arithmetic of direct_cluster_map_integrate_scan (include/direct_cluster.h, "one sensor scan folded into the map"): the voxels a
// ray from the sensor's origin to a return passes, the voxel of the return, and the box dilation of the scan grid that becomes
// the map.  Plain C++ behind a qualifier macro: the kernels of map_scan.h call these functions, and g++ compiles the same header
// for the CPU tests (tests/map_scan_harness.py).  There is no reference counterpart: the reference builds its map once
// (rcvPointCloudCallBack returns at once when it has one) and never takes a voxel out again.
//
// THE WALK.  All arithmetic in double, no square root (the device's fp64 square root has been measured one ulp off the host's,
// DESIGN.md 6.6); divisions are correctly rounded on both sides.  With inv = 1.0 / resolution computed once, R2 = max_range *
// max_range computed once on the host, e_a = (double)p_a of a float point p, d_a = e_a - o_a and dd = (d_x*d_x + d_y*d_y) + d_z*d_z:
//   hit        dd <= R2.  The ray ends in the voxel j_a = (int)floor((e_a - lower_a) * inv) of its point, which is "inside" when
//              0 <= j_a < size_a for all a; n_a = |j_a - i_a| steps are taken along axis a, no more and no fewer.
//   truncated  otherwise: the ray carves out to max_range and marks nothing.
//   start      i_a = axis_index_drop(o_a, ...) of map_cloud_math.h, computed and checked on the host (Grid::start).
//   per axis   step_a = sign(d_a); for step_a != 0: b = lower_a + (double)(i_a + (step_a > 0)) * resolution,
//              tmax_a = (b - o_a) / d_a, tdel_a = resolution / fabs(d_a).  An axis with step_a == 0 is never chosen.
//   loop       stop without writing when the current voxel is outside the map (the origin is inside and the map is convex: the
//              walk never comes back); a hit stops when n_x + n_y + n_z steps are done; choose the axis with the smallest tmax
//              among those with step != 0 and, for a hit, n_a > 0 (ties go to the lower axis); clear the current voxel; a
//              truncated ray stops here when !((t*t)*dd <= R2) for the chosen t = tmax_a; then i_a += step_a, tmax_a += tdel_a,
//              n_a -= 1.
// A hit thus clears every voxel before j and ends in j exactly, by COUNTING, whatever rounding does to a point on a voxel face;
// it does not clear j (the mark phase writes it).  A truncated ray clears its last voxel too.  Every loop is bounded: by
// n_x + n_y + n_z for a hit, by size_x + size_y + size_z for a truncated ray.  A point with a non-finite coordinate contributes
// nothing (is_finite3).  A hit's j fits an int because the caller refuses max_range * inv above kMaxRangeVox and the origin lies in
// the map; a truncated ray never computes j.
//
// Contraction: b and dd are sums of products, where a fused multiply-add would round once and move a tmax or a range test by an
// ulp.  This header switches contraction off itself, per function, as map_cloud_math.h does; under g++ the harness passes
// -ffp-contract=off.
//
// THE KNOWN GRID (flags & kTrackKnown) is a second byte per voxel, 1 = observed: every voxel carve_ray hands to `clear` and every
// voxel mark_voxel returns gets known = 1, at the same voxel() index (the callers write both bytes from the one lambda, there is
// no second walk).  Every writer of the known grid writes 1, in both phases: it depends neither on the order of the points nor
// on the launch shape, and needs no ordering between the phases.
//
// THE DILATION is a voxel box without wrap, separable: along one axis, dst is 1 exactly when some src voxel within r steps
// inside the map is 1.  Integers only.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "map_cloud_math.h"

namespace direct {
namespace mapscan {

constexpr int kMaxRangeVox = 4096;  // the library refuses max_range * inv above this
constexpr int kMaxInflate = 64;     // ... and an inflate above this
constexpr int kSkipped = 0, kHit = 1, kTruncated = 2;  // what classify() returns
constexpr int kTrackKnown = 1;      // direct_map_scan_t.flags, DIRECT_SCAN_TRACK_KNOWN; every other bit is refused
DIRECT_MAPCLOUD_HD bool flags_known(int flags) { return (flags & ~kTrackKnown) == 0; }

struct Grid {
  double lower[3], origin[3];
  double resolution, inv, R2;
  int size[3];
  int start[3];  // the origin's voxel (axis_index_drop), inside the map
};

DIRECT_MAPCLOUD_HD bool inside(const Grid& G, const int* v) {
  return v[0] >= 0 && v[0] < G.size[0] && v[1] >= 0 && v[1] < G.size[1] && v[2] >= 0 && v[2] < G.size[2];
}
DIRECT_MAPCLOUD_HD size_t voxel(const Grid& G, const int* v) {
  return ((size_t)v[0] * G.size[1] + v[1]) * G.size[2] + v[2];
}

// d and dd of a point; kSkipped, kHit or kTruncated
DIRECT_MAPCLOUD_HD int classify(const Grid& G, float x, float y, float z, double* e, double* d, double* dd) {
  DIRECT_MAPCLOUD_NO_CONTRACT
  if (!mapcloud::is_finite3(x, y, z)) return kSkipped;
  e[0] = (double)x; e[1] = (double)y; e[2] = (double)z;
  for (int a = 0; a < 3; a++) d[a] = e[a] - G.origin[a];
  const double xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
  *dd = (xx + yy) + zz;
  return *dd <= G.R2 ? kHit : kTruncated;
}

// the voxel of a hit's point; it may lie outside the map
DIRECT_MAPCLOUD_HD void end_voxel(const Grid& G, const double* e, int* j) {
  DIRECT_MAPCLOUD_NO_CONTRACT
  for (int a = 0; a < 3; a++) j[a] = (int)floor((e[a] - G.lower[a]) * G.inv);
}

// The carve phase of one point: clear(linear voxel index) for every voxel the ray passes.  -> classify()'s value
template <class Clear>
DIRECT_MAPCLOUD_HD int carve_ray(const Grid& G, float x, float y, float z, Clear clear) {
  DIRECT_MAPCLOUD_NO_CONTRACT
  double e[3], d[3], dd;
  const int kind = classify(G, x, y, z, e, d, &dd);
  if (kind == kSkipped) return kind;
  const bool hit = kind == kHit;
  int i[3], j[3], step[3], n[3] = {0, 0, 0};
  double tmax[3] = {0.0, 0.0, 0.0}, tdel[3] = {0.0, 0.0, 0.0};
  if (hit) end_voxel(G, e, j);
  long long bound = 0;
  for (int a = 0; a < 3; a++) {
    i[a] = G.start[a];
    step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
    if (hit) n[a] = j[a] > i[a] ? j[a] - i[a] : i[a] - j[a];
    bound += hit ? n[a] : G.size[a];
    if (step[a] != 0) {
      const double faces = (double)(i[a] + (step[a] > 0 ? 1 : 0)) * G.resolution;
      const double b = G.lower[a] + faces;
      tmax[a] = (b - G.origin[a]) / d[a];
      tdel[a] = G.resolution / fabs(d[a]);
    }
  }
  for (long long k = 0; k < bound; k++) {
    if (!inside(G, i)) break;
    int c = -1;
    for (int a = 0; a < 3; a++)
      if (step[a] != 0 && (!hit || n[a] > 0) && (c < 0 || tmax[a] < tmax[c])) c = a;
    if (c < 0) break;  // cannot happen: a hit with steps left has an axis with n > 0, a truncated ray has dd > 0
    clear(voxel(G, i));
    const double t = tmax[c];
    if (!hit && !((t * t) * dd <= G.R2)) break;
    i[c] += step[c];
    tmax[c] += tdel[c];
    n[c] -= 1;
  }
  return kind;
}

// The mark phase of one point.  -> 1: *at is the voxel to set; 0: nothing to mark (skipped or truncated); -1: a hit outside the map
DIRECT_MAPCLOUD_HD int mark_voxel(const Grid& G, float x, float y, float z, size_t* at) {
  double e[3], d[3], dd;
  if (classify(G, x, y, z, e, d, &dd) != kHit) return 0;
  int j[3];
  end_voxel(G, e, j);
  if (!inside(G, j)) return -1;
  *at = voxel(G, j);
  return 1;
}

// One voxel of one pass of the dilation along `axis` by r steps: v = (x, y, z) in a grid of `size`
DIRECT_MAPCLOUD_HD uint8_t dilate_at(const uint8_t* src, const int* size, int axis, int r, const int* v) {
  const size_t pitch = axis == 0 ? (size_t)size[1] * size[2] : (axis == 1 ? (size_t)size[2] : 1);
  const size_t at = ((size_t)v[0] * size[1] + v[1]) * size[2] + v[2];
  const int lo = v[axis] - r > 0 ? v[axis] - r : 0, hi = v[axis] + r < size[axis] - 1 ? v[axis] + r : size[axis] - 1;
  const uint8_t* q = src + at - (size_t)(v[axis] - lo) * pitch;
  for (int k = lo; k <= hi; k++, q += pitch)
    if (*q == 1) return 1;
  return 0;
}

}  // namespace mapscan
}  // namespace direct
