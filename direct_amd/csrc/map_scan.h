// Kernels of direct_cluster_map_integrate_scan (include/direct_cluster.h, "one sensor scan folded into the map"); included by
// direct_cluster.hip inside its anonymous namespace.  The arithmetic is map_scan_math.h's, shared with the CPU tests.
//
// One scan is carve, mark, inflate, in that order on the handle's stream:
//   k_scan_carve   a lane owns one ray and walks it, storing the byte 0 into the scan grid.  Every writer of this phase writes 0.
//   k_scan_mark    a lane owns one point and stores the byte 1 into its voxel; no walk.  Every writer of this phase writes 1, and
//                  the phase starts when the carve has ended: the scan grid depends neither on the order of the points nor on the
//                  launch shape, and the returns of this scan survive it.
//   k_scan_dilate  one pass of the separable box dilation along one axis; the LAST pass (x) writes the map, compares it with the
//                  byte the map held before and counts the two kinds of change, the map's ones and the scan grid's ones.
// Neighbouring points of a real scan walk neighbouring voxels and every ray crosses the voxels around the origin; the launch
// file's map (3.7 MB) fits one XCD's 4 MB L2, which absorbs the scatter.  kTest chooses between storing 0 unconditionally and
// loading the byte first and storing only where it is not 0 yet (tools/map_scan_bench.py times both).
// kKnown (DIRECT_SCAN_TRACK_KNOWN) adds the known grid: the carve's lambda and the mark store the byte 1 into it at the very index
// they write the scan grid at, under the same kTest choice.  Every writer of the known grid writes 1, in both phases: the known
// grid depends neither on the order of the points nor on the launch shape.  kKnown = false is the code without the known grid.
// k_known_set copies a caller's known grid in, one lane per voxel, as src != 0.
// Counters: one shuffle reduction per wave, then one 64-bit integer atomic per wave and counter, as in k_cloud_raster.
#pragma once
#include "map_scan_math.h"

namespace ms = direct::mapscan;

constexpr int kScanMaxBlocks = 1024;  // the grid-stride loops take a second trip beyond 262144 rays or voxels
enum { kScanSkipped = 0, kScanTruncated, kScanOutside, kScanRawOnes, kScanMapOnes, kScanSet, kScanCleared, kScanCounters };

struct ScanDev {
  ms::Grid G;
  long long n;             // points
  int stride;
  const float* xyz;        // [n][stride]
  uint8_t* raw;            // the scan grid, [size[0] * size[1] * size[2]]
  unsigned long long* cnt; // [kScanCounters]
  uint8_t* known;          // the known grid in the scan grid's layout; read and written by the kKnown instantiations only
};

__device__ __forceinline__ void scan_count(unsigned long long v, unsigned long long* where) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(where, v);
}

template <bool kTest, bool kKnown>
__global__ __launch_bounds__(256) void k_scan_carve(ScanDev S) {
  unsigned long long skipped = 0, truncated = 0;
  uint8_t* raw = S.raw;
  uint8_t* known = S.known;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < S.n; p += (long long)gridDim.x * blockDim.x) {
    const float* q = S.xyz + p * S.stride;
    const int kind = ms::carve_ray(S.G, q[0], q[1], q[2], [raw, known](size_t at) {
      if (!kTest || raw[at] != 0) raw[at] = 0;
      if (kKnown && (!kTest || known[at] != 1)) known[at] = 1;
    });
    skipped += kind == ms::kSkipped;
    truncated += kind == ms::kTruncated;
  }
  scan_count(skipped, &S.cnt[kScanSkipped]);
  scan_count(truncated, &S.cnt[kScanTruncated]);
}

template <bool kKnown>
__global__ __launch_bounds__(256) void k_scan_mark(ScanDev S) {
  unsigned long long outside = 0;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < S.n; p += (long long)gridDim.x * blockDim.x) {
    const float* q = S.xyz + p * S.stride;
    size_t at = 0;
    const int m = ms::mark_voxel(S.G, q[0], q[1], q[2], &at);
    if (m > 0) S.raw[at] = 1;
    if (kKnown && m > 0) S.known[at] = 1;
    outside += m < 0;
  }
  scan_count(outside, &S.cnt[kScanOutside]);
}

__global__ __launch_bounds__(256) void k_known_set(uint8_t* known, const uint8_t* src, long long G) {
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < G; t += (long long)gridDim.x * blockDim.x) known[t] = src[t] != 0;
}

struct DilateDev {
  int size[3];
  int axis, r;
  long long G;
  const uint8_t* src;
  uint8_t* dst;
  const uint8_t* raw;      // last pass only (else null): the scan grid, whose ones are counted, and dst is the map
  unsigned long long* cnt;
};

__global__ __launch_bounds__(256) void k_scan_dilate(DilateDev P) {
  unsigned long long raw_ones = 0, map_ones = 0, set = 0, cleared = 0;
  const int yz = P.size[1] * P.size[2];
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < P.G; t += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(t / yz), rem = (int)(t - (long long)x * yz);
    const int v[3] = {x, rem / P.size[2], rem % P.size[2]};
    const uint8_t now = ms::dilate_at(P.src, P.size, P.axis, P.r, v);
    if (P.raw) {
      const uint8_t before = P.dst[t];
      raw_ones += P.raw[t] == 1;
      map_ones += now;
      set += before != now && now == 1;
      cleared += before != now && now == 0;
      if (before != now) P.dst[t] = now;
    } else {
      P.dst[t] = now;
    }
  }
  if (P.raw) {  // uniform over the launch
    scan_count(raw_ones, &P.cnt[kScanRawOnes]);
    scan_count(map_ones, &P.cnt[kScanMapOnes]);
    scan_count(set, &P.cnt[kScanSet]);
    scan_count(cleared, &P.cnt[kScanCleared]);
  }
}
