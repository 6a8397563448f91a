// Kernels of direct_cluster_frontier (include/direct_cluster.h, "frontier goals"); included by direct_cluster.hip inside its
// anonymous namespace, behind free_comp.h and map_scan.h.  The rules are frontier_math.h's, shared with the CPU tests.  In order on
// the handle's stream, the kernel boundaries being the only ordering between them:
//   k_front_mask     one lane per voxel: the mask byte, 0 on frontier voxels and 1 elsewhere, and the counts of known and of
//                    frontier voxels (scan_count: a wave reduction, then one atomic per wave and counter).
//   free_comp_launch AS IT STANDS on CompDev{map = mask, d2 = null, min_d2 = 0} with this call's own label, size and counter
//                    words: enterable(mask, ...) is "is a frontier voxel".  The free-space labels of the handle are not touched.
//   k_front_count    per workgroup of 256 voxels the number of kept roots (label[v] == v && size[v] >= min_size), block_scan256.
//   k_front_scan     ONE wave: the exclusive scan of the workgroup counts in place, and their total, the kept components.  A lane
//                    owns a contiguous run of (counts + 63) / 64 words: 40 x 36 x 20 voxels are 113 counts, two words a lane.
//   k_front_scatter  the kept roots in ascending index take the slots 0, 1, ...: label and size of the first `capacity` go to the
//                    slot arrays, and every root's word of the slot grid gets its slot, or -1 (not kept, or beyond capacity).  Only
//                    roots' words of that grid are ever read, and this kernel writes every one of them: it needs no clear.
//   k_front_sum      a frontier voxel of a written component adds its coordinates to its slot's sums: one packed 64-bit wave
//                    reduction and three atomics per DISTINCT slot of a wave (the ballot loop of k_cc_flatten).
//   k_front_rep      every such voxel forms its key against its slot's centroid voxel: one 64-bit atomicMin per distinct slot of
//                    a wave.
//   k_front_unpack   one lane per written slot: label, size, centroid and representative to the caller's arrays.
// Every per-voxel kernel runs one workgroup per 256 voxels and is not grid-strided: there is no second-trip path.  No wave waits
// for another; the ballot loops end within 64 turns (a turn retires at least its leader), k_front_scan's within its run.  Sums and
// minima are order-independent integers: no output depends on the launch shape.
#pragma once
#include "frontier_math.h"

namespace fr = ::direct::frontier;

enum { kFrontKnown = 0, kFrontVoxels, kFrontKept, kFrontCounters };

struct FrontDev {
  const uint8_t *map, *known;
  const int32_t* d2;           // the stored field; not read without a floor
  uint8_t* mask;               // [G]
  int32_t *label, *size;       // [G] the labelling's outputs
  int32_t* slot;               // [G] root -> slot or -1; words of other voxels hold anything
  int32_t* wg;                 // [nb] kept roots per workgroup, then their exclusive scan
  unsigned long long* cnt;     // [kFrontCounters]
  int32_t *s_label, *s_size;   // [capacity]
  unsigned long long* s_sum;   // [capacity][3], cleared to 0
  unsigned long long* s_key;   // [capacity], cleared to fr::kNoKey
  int32_t *o_label, *o_size, *o_centroid, *o_rep;  // the caller's arrays (or their staging), any may be null
  int X, Y, Z, G, nb, min_d2, min_size, capacity;
};

__device__ __forceinline__ void front_xyz(const FrontDev& F, int g, int& x, int& y, int& z) {
  const int YZ = F.Y * F.Z;
  x = g / YZ;
  y = (g / F.Z) % F.Y;
  z = g % F.Z;
}
__device__ __forceinline__ int front_written(const FrontDev& F) {
  const unsigned long long kept = F.cnt[kFrontKept];
  return kept < (unsigned long long)F.capacity ? (int)kept : F.capacity;
}
// the slot of voxel g's component when it is a written one, else -1
__device__ __forceinline__ int front_slot(const FrontDev& F, long long g) {
  if (g >= F.G) return -1;
  const int r = F.label[g];
  return r < 0 ? -1 : F.slot[r];
}

__global__ __launch_bounds__(256) void k_front_mask(FrontDev F) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned long long known = 0, front = 0;
  if (g < F.G) {
    int x, y, z;
    front_xyz(F, (int)g, x, y, z);
    const uint8_t m = fr::mask_byte(F.map, F.known, F.d2, x, y, z, F.X, F.Y, F.Z, F.min_d2);
    F.mask[g] = m;
    known = F.known[g] != 0;
    front = m == 0;
  }
  scan_count(known, &F.cnt[kFrontKnown]);
  scan_count(front, &F.cnt[kFrontVoxels]);
}

__global__ __launch_bounds__(256) void k_front_count(FrontDev F) {
  __shared__ int wsum[4];
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int flag = g < F.G && fr::kept_root(F.label[g], F.size[g], g, F.min_size);
  int tot;
  block_scan256(flag, &tot, wsum);
  if (threadIdx.x == 0) F.wg[blockIdx.x] = tot;
}

__global__ __launch_bounds__(64) void k_front_scan(FrontDev F) {
  const int lane = threadIdx.x, run = (F.nb + 63) / 64;
  const int lo = lane * run < F.nb ? lane * run : F.nb, hi = lo + run < F.nb ? lo + run : F.nb;
  int sum = 0;
  for (int i = lo; i < hi; i++) sum += F.wg[i];
  int inc = sum;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  int before = inc - sum;
  for (int i = lo; i < hi; i++) {
    const int c = F.wg[i];
    F.wg[i] = before;
    before += c;
  }
  if (lane == 63) F.cnt[kFrontKept] = (unsigned long long)inc;
}

__global__ __launch_bounds__(256) void k_front_scatter(FrontDev F) {
  __shared__ int wsum[4];
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool root = g < F.G && F.label[g] == (int32_t)g;
  const int flag = root && fr::kept_root(F.label[g], F.size[g], g, F.min_size);
  int tot;
  const int s = F.wg[blockIdx.x] + block_scan256(flag, &tot, wsum);
  if (!root) return;
  const bool written = flag && s < F.capacity;
  F.slot[g] = written ? s : -1;
  if (written) {
    F.s_label[s] = (int32_t)g;
    F.s_size[s] = F.size[g];
  }
}

__global__ __launch_bounds__(256) void k_front_sum(FrontDev F) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int s = front_slot(F, g);
  unsigned long long mine = 0;
  if (s >= 0) {
    int x, y, z;
    front_xyz(F, (int)g, x, y, z);
    mine = fr::pack_xyz(x, y, z);
  }
  unsigned long long todo = __ballot(s >= 0);
  for (int turn = 0; turn < 64 && todo; turn++) {
    const int lead = __ffsll((long long)todo) - 1;
    const int s0 = __shfl(s, lead);
    const unsigned long long same = __ballot(s == s0) & todo;
    unsigned long long v = s == s0 ? mine : 0;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == lead)
      for (int a = 0; a < 3; a++) atomicAdd(&F.s_sum[3 * (size_t)s0 + a], (unsigned long long)fr::packed_axis(v, a));
    todo &= ~same;
  }
}

__device__ __forceinline__ void front_centroid(const FrontDev& F, int s, int32_t* c) {
  const long long n = F.s_size[s];
  for (int a = 0; a < 3; a++) c[a] = fr::centroid_axis((long long)F.s_sum[3 * (size_t)s + a], n);
}

__global__ __launch_bounds__(256) void k_front_rep(FrontDev F) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int s = front_slot(F, g);
  unsigned long long mine = fr::kNoKey;
  if (s >= 0) {
    int x, y, z;
    int32_t c[3];
    front_xyz(F, (int)g, x, y, z);
    front_centroid(F, s, c);
    mine = fr::rep_key(x, y, z, c, g);
  }
  unsigned long long todo = __ballot(s >= 0);
  for (int turn = 0; turn < 64 && todo; turn++) {
    const int lead = __ffsll((long long)todo) - 1;
    const int s0 = __shfl(s, lead);
    const unsigned long long same = __ballot(s == s0) & todo;
    unsigned long long v = s == s0 ? mine : fr::kNoKey;
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(v, o);
      v = other < v ? other : v;
    }
    if (lane == lead) atomicMin(&F.s_key[s0], v);
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void k_front_unpack(FrontDev F) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= front_written(F)) return;
  if (F.o_label) F.o_label[s] = F.s_label[s];
  if (F.o_size) F.o_size[s] = F.s_size[s];
  if (F.o_centroid) front_centroid(F, s, F.o_centroid + 3 * (size_t)s);
  if (F.o_rep) {
    int x, y, z;
    front_xyz(F, fr::key_voxel(F.s_key[s]), x, y, z);
    F.o_rep[3 * (size_t)s] = x;
    F.o_rep[3 * (size_t)s + 1] = y;
    F.o_rep[3 * (size_t)s + 2] = z;
  }
}

// Enqueues everything behind the labelling; the slot sums and keys have been cleared on the same stream.
inline hipError_t front_compact_launch(const FrontDev& F, hipStream_t stream) {
  hipLaunchKernelGGL(k_front_count, dim3(F.nb), dim3(256), 0, stream, F);
  hipLaunchKernelGGL(k_front_scan, dim3(1), dim3(64), 0, stream, F);
  hipLaunchKernelGGL(k_front_scatter, dim3(F.nb), dim3(256), 0, stream, F);
  return hipGetLastError();
}
inline hipError_t front_goals_launch(const FrontDev& F, hipStream_t stream) {
  if (F.capacity == 0) return hipSuccess;
  hipLaunchKernelGGL(k_front_sum, dim3(F.nb), dim3(256), 0, stream, F);
  hipLaunchKernelGGL(k_front_rep, dim3(F.nb), dim3(256), 0, stream, F);
  hipLaunchKernelGGL(k_front_unpack, dim3((F.capacity + 255) / 256), dim3(256), 0, stream, F);
  return hipGetLastError();
}
