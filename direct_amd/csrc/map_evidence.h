// Kernels of direct_cluster_map_integrate_scan_evidence (include/direct_cluster.h, "occupancy evidence per voxel"); included by
// direct_cluster.hip inside its anonymous namespace, behind map_scan.h.  The arithmetic is map_evidence_math.h's and the walk is
// map_scan_math.h's, both shared with the CPU tests.
//
// One evidence scan is touch, hit, fold, inflate, in that order on the handle's stream:
//   k_evid_touch  a lane owns one ray and walks it with ms::carve_ray, storing the byte 1 into the TOUCH grid: exactly the voxels
//                 the plain carve would clear.  The byte is loaded first and stored only where it is not 1 yet (the tested-store
//                 form of k_scan_carve).  Every writer of this phase writes 1.
//   k_evid_hit    a lane owns one point and stores the byte 2 into the touch byte of its voxel; no walk.  Every writer of this
//                 phase writes 2 and the phase starts when the touch phase has ended: a voxel both passed and hit is a hit, and the
//                 touch grid depends neither on the order of the points nor on the launch shape.
//   k_evid_fold   one pass over the grid, the only one that reads or writes the evidence: a lane owns 16 consecutive voxels and
//                 moves touch, evidence, scan grid and (tracked) known grid as one 128-bit word each.  A group of evidence, scan
//                 grid or known grid is stored only when it changed: a static scene that has saturated writes nothing.  The last
//                 group of a grid whose voxel count is no multiple of 16 goes byte by byte and never reads past the end.
//                 kAdopt takes the evidence from the map's bytes (DIRECT_SCAN_ADOPT; the map is not written before the last
//                 dilation pass) and then always stores it.
// The dilation and its counters are k_scan_dilate's, untouched.  The touch grid has no storage of its own: it is dead once the fold
// has run, and lives in the first `cells` bytes of the dilation workspace, which the z and y passes only write afterwards.
// Every loop is bounded; no LDS, no waiting between waves.  Counters go through scan_count.
#pragma once
#include "map_evidence_math.h"
#include "map_scan.h"

namespace me = direct::mapevid;

constexpr int kEvidGroup = 16;  // voxels per lane and trip of the fold: one 128-bit word per grid
enum { kEvidHit = 0, kEvidPass, kEvidPositive, kEvidNegative, kEvidCounters };

template <bool kTest>
__global__ __launch_bounds__(256) void k_evid_touch(ScanDev S, uint8_t* touch) {
  unsigned long long skipped = 0, truncated = 0;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < S.n; p += (long long)gridDim.x * blockDim.x) {
    const float* q = S.xyz + p * S.stride;
    const int kind = ms::carve_ray(S.G, q[0], q[1], q[2], [touch](size_t at) {
      if (!kTest || touch[at] != me::kPass) touch[at] = me::kPass;
    });
    skipped += kind == ms::kSkipped;
    truncated += kind == ms::kTruncated;
  }
  scan_count(skipped, &S.cnt[kScanSkipped]);
  scan_count(truncated, &S.cnt[kScanTruncated]);
}

__global__ __launch_bounds__(256) void k_evid_hit(ScanDev S, uint8_t* touch) {
  unsigned long long outside = 0;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < S.n; p += (long long)gridDim.x * blockDim.x) {
    const float* q = S.xyz + p * S.stride;
    size_t at = 0;
    const int m = ms::mark_voxel(S.G, q[0], q[1], q[2], &at);
    if (m > 0) touch[at] = me::kHit;
    outside += m < 0;
  }
  scan_count(outside, &S.cnt[kScanOutside]);
}

struct EvidDev {
  me::Params P;
  long long G;                // voxels
  const uint8_t* touch;       // [G] 0, 1 or 2
  int8_t* ev;                 // [G] the evidence grid
  const uint8_t* map;         // kAdopt only: the map, whose bytes give the evidence the fold starts from
  uint8_t* raw;               // [G] the scan grid: (ev >= occ) of every voxel behind the fold
  uint8_t* known;             // kKnown only: known |= touch != 0
  unsigned long long* cnt;    // [kEvidCounters]
};

struct Evid16 { uint32_t w[4]; };  // 16 bytes of a grid, byte k of the group in bits 8 * (k % 4) of word k / 4

// n == 16: one 128-bit load (the grids are 256-byte aligned and a group starts at a multiple of 16); n < 16, the tail: n bytes
__device__ __forceinline__ Evid16 evid_load(const uint8_t* p, int n) {
  Evid16 r = {{0u, 0u, 0u, 0u}};
  if (n == kEvidGroup) {
    const uint4 q = *(const uint4*)p;
    r.w[0] = q.x; r.w[1] = q.y; r.w[2] = q.z; r.w[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < kEvidGroup; k++)
      if (k < n) r.w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
  }
  return r;
}
__device__ __forceinline__ void evid_store(uint8_t* p, int n, const Evid16& v) {
  if (n == kEvidGroup) {
    *(uint4*)p = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kEvidGroup; k++)
      if (k < n) p[k] = (uint8_t)(v.w[k >> 2] >> (8 * (k & 3)));
  }
}
__device__ __forceinline__ bool evid_differ(const Evid16& a, const Evid16& b) {
  return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3])) != 0u;
}

template <bool kAdopt, bool kKnown>
__global__ __launch_bounds__(256) void k_evid_fold(EvidDev E) {
  unsigned long long hits = 0, passes = 0, positive = 0, negative = 0;
  const long long groups = (E.G + kEvidGroup - 1) / kEvidGroup;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
    const long long at = g * kEvidGroup;
    const int n = E.G - at < kEvidGroup ? (int)(E.G - at) : kEvidGroup;
    const Evid16 t = evid_load(E.touch + at, n);
    const Evid16 e0 = evid_load(kAdopt ? E.map + at : (const uint8_t*)E.ev + at, n);
    const Evid16 r0 = evid_load(E.raw + at, n);
    Evid16 k0 = {{0u, 0u, 0u, 0u}};
    if (kKnown) k0 = evid_load(E.known + at, n);
    Evid16 e1 = {{0u, 0u, 0u, 0u}}, r1 = e1, k1 = k0;
#pragma unroll
    for (int k = 0; k < kEvidGroup; k++) {
      const int w = k >> 2, sh = 8 * (k & 3);
      const int tk = (int)((t.w[w] >> sh) & 0xffu);
      const uint32_t byte = (e0.w[w] >> sh) & 0xffu;
      const int before = kAdopt ? me::adopt((uint8_t)byte, E.P) : (int)(int8_t)byte;
      const int e = me::fold(before, tk, E.P);
      const bool live = k < n;  // the bytes behind the end of the tail are zero in every word and stay so
      e1.w[w] |= live ? ((uint32_t)e & 0xffu) << sh : 0u;
      r1.w[w] |= live && me::occupied(e, E.P) ? 1u << sh : 0u;
      if (kKnown) k1.w[w] |= live && tk != me::kNone ? 1u << sh : 0u;
      hits += live && tk == me::kHit;
      passes += live && tk == me::kPass;
      positive += live && e > 0;
      negative += live && e < 0;
    }
    if (kAdopt || evid_differ(e0, e1)) evid_store((uint8_t*)E.ev + at, n, e1);
    if (evid_differ(r0, r1)) evid_store(E.raw + at, n, r1);
    if (kKnown && evid_differ(k0, k1)) evid_store(E.known + at, n, k1);
  }
  scan_count(hits, &E.cnt[kEvidHit]);
  scan_count(passes, &E.cnt[kEvidPass]);
  scan_count(positive, &E.cnt[kEvidPositive]);
  scan_count(negative, &E.cnt[kEvidNegative]);
}

// set_evidence: the caller's bytes with -128 pulled to -127, one lane per voxel
__global__ __launch_bounds__(256) void k_evid_set(int8_t* ev, const int8_t* src, long long G) {
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < G; t += (long long)gridDim.x * blockDim.x) ev[t] = me::store_clamp(src[t]);
}
