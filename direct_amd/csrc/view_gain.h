// Kernel of direct_cluster_view_gain_batch (include/direct_cluster.h, "visible unknown volume per candidate viewpoint"); included
// by direct_cluster.hip inside its anonymous namespace.  The walk and the box are view_gain_math.h's, shared with the CPU tests.
//
// k_view_gain: ONE workgroup per candidate.  The candidate's code is uniform over the workgroup, so a candidate that is not OK
// returns as a whole before any barrier.  Otherwise the workgroup clears its box of (2R+1)^3 bits in LDS (dynamic, sized from R:
// short ranges keep several workgroups on a CU) and its six counters, and the rays of the candidate's direction set are strided
// over the lanes.  A lane that visits a voxel READS the word first and leaves a voxel whose bit is set alone (bits are only ever
// set between the two barriers, so a set bit read is a set bit: every ray starts in v0 and neighbouring rays share their first
// voxels, where plain reads of one address broadcast and atomics on it would queue); else a returning LDS atomic OR decides: the
// ONE lane that gets the bit back clear counts the voxel as seen and, after loading its known byte, as gain.  A lane's counts are
// reduced over its wave by shuffles, added to the LDS counters by one lane per wave, and written by vector stores behind the second
// barrier.  No wave waits for another beyond the two workgroup barriers; sums of first-setter counts do not depend on who came
// first: no output depends on the launch shape.
// An offset outside the box and a walk past its trip bound cannot happen; both set a bit of the error word and touch nothing.
#pragma once
#include "view_gain_math.h"

namespace vg = direct::viewgain;

// Threads per workgroup.  1024: the walk is a chain of dependent double operations ended by a byte load of the map that the next
// step's branch waits for, so other waves are the only latency hiding, and a candidate's rays are the only parallelism a
// workgroup has.  Measured against 256 and 512: never slower, up to three times faster where the box leaves one
// workgroup on a CU.
constexpr int kViewThreads = 1024;

struct ViewDev {
  vg::Scene S;
  const uint8_t *map, *known;
  const int32_t* voxel;   // [n][3]
  const int32_t* set;     // [n] or null: all 0
  const float* dirs;      // [n_sets][n_dirs][3]
  int32_t *code, *gain, *seen, *ends;  // [n], [n], [n], [n][4]; any may be null
  unsigned int* err;      // the error word
  int n_dirs, n_sets, words;
};

__global__ __launch_bounds__(kViewThreads) void k_view_gain(ViewDev V) {
  extern __shared__ unsigned int view_bits[];  // [V.words] the candidate's box
  __shared__ int s_cnt[2 + vg::kEnds];         // seen, gain, ends[4]
  const size_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const int v0[3] = {V.voxel[3 * c], V.voxel[3 * c + 1], V.voxel[3 * c + 2]};
  const int set = V.set ? V.set[c] : 0;
  const int code = vg::candidate_code(V.S, V.map, v0, set, V.n_sets);
  if (code != vg::kOk) {  // uniform over the workgroup
    if (tid == 0) {
      if (V.code) V.code[c] = code;
      if (V.gain) V.gain[c] = 0;
      if (V.seen) V.seen[c] = 0;
    }
    if (tid < vg::kEnds && V.ends) V.ends[4 * c + tid] = 0;
    return;
  }
  for (int w = tid; w < V.words; w += blockDim.x) view_bits[w] = 0u;
  if (tid < 2 + vg::kEnds) s_cnt[tid] = 0;
  __syncthreads();
  int cnt[2 + vg::kEnds] = {0, 0, 0, 0, 0, 0};
  unsigned int err = 0;
  const float* dirs = V.dirs + (size_t)set * V.n_dirs * 3;
  const uint8_t* known = V.known;
  const int R = V.S.R;
  for (int r = tid; r < V.n_dirs; r += blockDim.x) {
    const float* q = dirs + 3 * (size_t)r;
    int seen = 0, gain = 0;
    const int end = vg::cast_ray(V.S, V.map, v0, q[0], q[1], q[2], [&](const int* i, size_t at) {
      const int bit = vg::box_bit(R, v0, i);
      if (bit < 0) {
        err |= vg::kErrBox;
        return;
      }
      const unsigned int m = 1u << (bit & 31);
      unsigned int* word = &view_bits[bit >> 5];
      if (*(volatile unsigned int*)word & m) return;
      if (atomicOr(word, m) & m) return;
      seen++;
      gain += known[at] == 0;
    });
    cnt[0] += seen;
    cnt[1] += gain;
    if (end < 0) err |= vg::kErrTrips;
    else
      for (int k = 0; k < vg::kEnds; k++) cnt[2 + k] += end == k;  // a constant index per turn: the counters stay in registers
  }
  for (int k = 0; k < 2 + vg::kEnds; k++) {
    int v = cnt[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0 && v) atomicAdd(&s_cnt[k], v);
  }
  if (err) atomicOr(V.err, err);
  __syncthreads();
  if (tid == 0) {
    if (V.code) V.code[c] = vg::kOk;
    if (V.seen) V.seen[c] = s_cnt[0];
    if (V.gain) V.gain[c] = s_cnt[1];
  }
  if (tid < vg::kEnds && V.ends) V.ends[4 * c + tid] = s_cnt[2 + tid];
}
