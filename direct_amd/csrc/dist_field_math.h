// Arithmetic of direct_cluster_distance_field (include/direct_cluster.h, "distance field of the resident map"): the three separable
// passes of the exact squared Euclidean distance transform, each as the work on ONE line.  Plain C++ behind a qualifier macro: the
// kernels of dist_field.h call these functions, and g++ compiles the same header for the CPU tests (tests/dist_field_harness.py).
//
//   D2[v] = min over occupied u of (vx-ux)^2 + (vy-uy)^2 + (vz-uz)^2
//         = min_ux ((vx-ux)^2 + min_uy ((vy-uy)^2 + min over occupied (ux, uy, uz) of (vz-uz)^2))
// so pass z gives every voxel the squared distance to the nearest occupied voxel of its own column, and passes y and x are
// out[i] = min_j (in[j] + (i-j)^2) over a line.  All integer; kNone stands for +infinity and is skipped as a source, never added to.
//
// The cap.  The stored value is min(D2, cap2).  Because (i-j)^2 >= 0, min(cap2, min_j (in[j] + (i-j)^2)) is the same number
// whether in[] is first capped or not, so pass z stores min(., cap2) and the later passes keep every value <= cap2 by starting
// from in[i]: capping early is exact, and it bounds the scan below by cap_vox steps.
//
// The scan (passes y and x).  Per output, best starts at in[i] and the candidates are visited outward, r = |i-j| = 1, 2, ...; the
// scan stops at the first r with r*r >= best.  Exact: every candidate not yet visited is in[j] + (i-j)^2 >= r*r >= best.  It is
// bounded by the line length, which is what an empty line costs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DIRECT_DISTFIELD_HD __host__ __device__ __forceinline__
#else
#define DIRECT_DISTFIELD_HD inline
#endif

namespace direct {
namespace distfield {

constexpr int kNone = 0x7fffffff;  // DIRECT_DIST_NONE: no occupied voxel
constexpr int kMaxCap = 1024;      // cap_vox above the largest dimension caps nothing

// cap2 of a cap_vox in [0, kMaxCap]
DIRECT_DISTFIELD_HD int cap2_of(int cap_vox) { return cap_vox > 0 ? cap_vox * cap_vox : kNone; }

// Pass z for one column of n map bytes m[k * sm]: out[k * so] = min(cap2, (k - k')^2) with k' the nearest k' whose byte is 1
// (kNone on a column without one when cap2 is kNone).  Two sweeps.
template <typename Byte, typename Int>
DIRECT_DISTFIELD_HD void pass_z(const Byte* m, int sm, int n, int cap2, Int* out, int so) {
  int d = -1;  // steps since the last occupied voxel below; -1: none
  for (int k = 0; k < n; k++) {
    d = m[k * sm] == 1 ? 0 : (d < 0 ? -1 : d + 1);
    const int v = d < 0 ? kNone : d * d;
    out[k * so] = v < cap2 ? v : cap2;
  }
  d = -1;
  for (int k = n - 1; k >= 0; k--) {
    d = m[k * sm] == 1 ? 0 : (d < 0 ? -1 : d + 1);
    const int v = d < 0 ? kNone : d * d;
    out[k * so] = v < out[k * so] ? v : (int)out[k * so];
  }
}

// One output of passes y and x: min_j (in[j * s] + (i-j)^2) over the line of n entries, by the outward scan
template <typename Int>
DIRECT_DISTFIELD_HD int scan_min(const Int* in, long long s, int n, int i) {
  int best = in[i * s];
  for (int r = 1; r < n; r++) {
    const int r2 = r * r;
    if (r2 >= best) break;
    if (i - r >= 0) {
      const int v = in[(i - r) * s];
      if (v != kNone && v + r2 < best) best = v + r2;
    }
    if (i + r < n) {
      const int v = in[(i + r) * s];
      if (v != kNone && v + r2 < best) best = v + r2;
    }
  }
  return best;
}

// The whole field on one thread, d2[X * Y * Z] from map[X * Y * Z]; tmp has the same size.  What the kernels must equal.
inline void field_host(const uint8_t* map, int X, int Y, int Z, int cap_vox, int32_t* d2, int32_t* tmp) {
  const int cap2 = cap2_of(cap_vox);
  const long long YZ = (long long)Y * Z;
  for (long long c = 0; c < (long long)X * Y; c++) pass_z(map + c * Z, 1, Z, cap2, d2 + c * Z, 1);
  for (int x = 0; x < X; x++)
    for (int y = 0; y < Y; y++)
      for (int z = 0; z < Z; z++) tmp[x * YZ + (long long)y * Z + z] = scan_min(d2 + x * YZ + z, (long long)Z, Y, y);
  for (int x = 0; x < X; x++)
    for (long long q = 0; q < YZ; q++) d2[x * YZ + q] = scan_min(tmp + q, YZ, X, x);
}

// stats of a finished field: [0] voxels with a stored value below cap2, [1] the largest such value or -1
inline void stats_host(const int32_t* d2, long long G, int cap_vox, int64_t* stats) {
  const int cap2 = cap2_of(cap_vox);
  stats[0] = 0;
  stats[1] = -1;
  for (long long g = 0; g < G; g++)
    if (d2[g] < cap2) {
      stats[0]++;
      if (d2[g] > stats[1]) stats[1] = d2[g];
    }
}

}  // namespace distfield
}  // namespace direct
