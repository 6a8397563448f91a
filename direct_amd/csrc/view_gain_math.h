// Arithmetic of direct_cluster_view_gain_batch (include/direct_cluster.h, "visible unknown volume per candidate viewpoint"): the
// voxels an ideal sensor's ray passes from the centre of a candidate voxel until it is blocked, leaves the map or runs out of
// range, and where each of them sits in the candidate's box of bits.  Plain C++ behind the qualifier macro of map_cloud_math.h:
// the kernel of view_gain.h calls these functions, and g++ compiles the same header for the CPU tests
// (tests/view_gain_harness.py).  There is no reference counterpart: the reference never ranks a goal by what it would see.
//
// THE WALK is the carve walk of map_scan_math.h for a truncated ray, in VOXEL units from the centre of v0, except that it stops
// at an occupied voxel.  All arithmetic in double, no square root; the division is correctly rounded on both sides.  With
// d_a = (double)dir_a of a float direction (any length), dd = (d_x*d_x + d_y*d_y) + d_z*d_z and R2 = range_vox * range_vox
// computed once on the host:
//   skipped    a component is not finite, or dd == 0.  Nothing is visited.
//   per axis   step_a = sign(d_a); for step_a != 0: tdel_a = 1.0 / fabs(d_a), tmax_a = 0.5 * tdel_a (the centre is half a voxel
//              from every face).  An axis with step_a == 0 is never chosen.
//   loop       i = v0; then, in this order: i outside the map -> LEFT (i is not visited); visit(i); map byte at i != 0 -> BLOCKED
//              (the voxel an ideal return would mark); c = the axis with the smallest tmax among those with step != 0, ties to the
//              lower axis; t = tmax_c, !((t*t)*dd <= R2) -> RANGE; i_c += step_c, tmax_c += tdel_c.
// t is the ray parameter at which the walk would leave the current voxel, t * sqrt(dd) the distance in voxels: a voxel is visited
// when the ray ENTERS it within range_vox.  No per-axis offset from v0 exceeds floor(range_vox + 0.5) (the face at offset k + 1/2
// is crossed at distance >= k + 1/2), which is at most R - 1 with R = (int)floor(range_vox) + 2: the visited voxels fit the box of
// side 2R + 1 around v0, and the walk takes at most 3(R - 1) steps.  The loop carries the trip bound 3R + 3 all the same; passing
// it, like an offset outside the box, is reported and never acted on.
//
// Contraction: dd and (t*t)*dd are products that feed sums or comparisons, where a fused multiply-add would round once and move a
// range test by an ulp.  Switched off per function, as in map_scan_math.h; under g++ the harness passes -ffp-contract=off.
//
// THE COUNTS of a candidate over all rays of its direction set: seen, the DISTINCT voxels visited; gain, those of them with
// known == 0; ends[4], the rays by outcome.  Distinctness is a bit per voxel of the box: the ONE visitor that finds the bit clear
// counts the voxel.  Sums of such counts depend neither on the order of the rays nor on who visits first.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "map_cloud_math.h"

namespace direct {
namespace viewgain {

constexpr int kMaxR = 50;         // the largest box half-width: (2 * 50 + 1)^3 bits are 128 792 bytes of the CU's 160 KiB
constexpr int kMaxDirs = 65536;   // rays per direction set
constexpr int kBlocked = 0, kLeft = 1, kRange = 2, kSkipped = 3, kEnds = 4;  // what cast_ray returns: the index into ends[4]
constexpr int kTripBound = -1;    // ... or this: the walk passed its trip bound (cannot happen)
constexpr int kOk = 0, kOutside = 1, kOccupied = 2, kBadSet = 3;             // DIRECT_VIEW_*, the per-candidate code
constexpr unsigned kErrBox = 1, kErrTrips = 2;                                // bits of the error word

// The box half-width of a range.  range_vox is finite and positive; the caller compares in double BEFORE converting
// (supported()), so the conversion is defined.
DIRECT_MAPCLOUD_HD bool supported(double range_vox) { return floor(range_vox) + 2.0 <= (double)kMaxR; }
DIRECT_MAPCLOUD_HD int box_half(double range_vox) { return (int)floor(range_vox) + 2; }
DIRECT_MAPCLOUD_HD int box_side(int R) { return 2 * R + 1; }
DIRECT_MAPCLOUD_HD int box_words(int R) { return (box_side(R) * box_side(R) * box_side(R) + 31) / 32; }

struct Scene {
  int size[3];  // the map
  int R;        // box_half(range_vox)
  double R2;    // range_vox * range_vox
};

DIRECT_MAPCLOUD_HD bool inside(const Scene& S, const int* v) {
  return v[0] >= 0 && v[0] < S.size[0] && v[1] >= 0 && v[1] < S.size[1] && v[2] >= 0 && v[2] < S.size[2];
}
DIRECT_MAPCLOUD_HD size_t voxel(const Scene& S, const int* v) {
  return ((size_t)v[0] * S.size[1] + v[1]) * S.size[2] + v[2];
}

// The code of a candidate, in the order of the table: outside the map, then occupied, then a set index outside [0, n_sets)
DIRECT_MAPCLOUD_HD int candidate_code(const Scene& S, const uint8_t* map, const int* v0, int set, int n_sets) {
  if (!inside(S, v0)) return kOutside;
  if (map[voxel(S, v0)] != 0) return kOccupied;
  if (set < 0 || set >= n_sets) return kBadSet;
  return kOk;
}

// The bit of voxel i in the box around v0, or -1 when an offset exceeds R (cannot happen for a voxel the walk visits)
DIRECT_MAPCLOUD_HD int box_bit(int R, const int* v0, const int* i) {
  const int side = box_side(R);
  const int ox = i[0] - v0[0] + R, oy = i[1] - v0[1] + R, oz = i[2] - v0[2] + R;
  if (ox < 0 || ox >= side || oy < 0 || oy >= side || oz < 0 || oz >= side) return -1;
  return (ox * side + oy) * side + oz;
}

// One ray from the centre of v0 (inside the map): visit(i, linear voxel index) for every voxel it passes.  -> kBlocked, kLeft,
// kRange, kSkipped, or kTripBound
template <class Visit>
DIRECT_MAPCLOUD_HD int cast_ray(const Scene& S, const uint8_t* map, const int* v0, float x, float y, float z, Visit visit) {
  DIRECT_MAPCLOUD_NO_CONTRACT
  if (!mapcloud::is_finite3(x, y, z)) return kSkipped;
  const double d[3] = {(double)x, (double)y, (double)z};
  const double xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
  const double dd = (xx + yy) + zz;
  if (dd == 0.0) return kSkipped;
  int i[3], step[3];
  double tmax[3] = {0.0, 0.0, 0.0}, tdel[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < 3; a++) {
    i[a] = v0[a];
    step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
    if (step[a] != 0) {
      tdel[a] = 1.0 / fabs(d[a]);
      tmax[a] = 0.5 * tdel[a];
    }
  }
  const int bound = 3 * S.R + 3;
  for (int k = 0; k < bound; k++) {
    if (!inside(S, i)) return kLeft;
    const size_t at = voxel(S, i);
    visit(i, at);
    if (map[at] != 0) return kBlocked;
    int c = -1;
    for (int a = 0; a < 3; a++)
      if (step[a] != 0 && (c < 0 || tmax[a] < tmax[c])) c = a;
    if (c < 0) return kTripBound;  // cannot happen: dd > 0 has an axis with a step
    const double t = tmax[c];
    if (!((t * t) * dd <= S.R2)) return kRange;
    i[c] += step[c];
    tmax[c] += tdel[c];
  }
  return kTripBound;
}

}  // namespace viewgain
}  // namespace direct
