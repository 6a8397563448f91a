// Kernels of direct_cluster_free_components and direct_cluster_reachable_batch (include/direct_cluster.h, "free-space
// components"); included by direct_cluster.hip inside its anonymous namespace.  The rules are free_comp_math.h's, shared with the
// CPU tests.  Five kernels, and the kernel boundaries are the only ordering between them:
//   k_cc_tile     one workgroup per 8^3 tile (partial tiles at the upper borders included): the enterable bits go to LDS as
//                 parent = self / -1, every voxel unites itself with its forward neighbours INSIDE the tile by a union-find on LDS
//                 words (atomicMin, parent <= self), and parent[v] = global index of the tile-local root goes out, -1 otherwise.
//                 Local and global indices order a tile's voxels alike, so the local root is the smallest global index.
//   k_cc_merge    one lane per voxel; a voxel on a tile face unites itself with every forward neighbour that lies in ANOTHER tile
//                 (face, edge and corner diagonals: one, two or three borders at once) and is enterable.  Every access to
//                 `parent` in this kernel is a relaxed agent-scope atomic (load or min), served by L2: no lane relies on another
//                 lane's progress, a stale value costs a turn of unite's loop (free_comp_math.h, I1 - I4).
//   k_cc_flatten  label[v] = root(v) by pointer chasing (indices fall strictly), written in place - a word is only ever replaced
//                 by an ancestor, so a chaser that meets it still arrives - and size_at_root[label] += 1.
//   k_cc_sizes    size[v] = size_at_root[label[v]] (a root's own word is read, never rewritten), and the stats: wave reductions,
//                 then one integer atomic per wave and counter.
//   k_reach       one lane per pair: free_comp_math.h's reach_pair on the labels, up to 26 label loads for a start that is not
//                 enterable.
// No persistent kernel, no wave waits for another, no floating point.  Every loop carries a trip bound (no chain is longer than the
// voxel count); passing it sets a bit of the sticky error word, which the host turns into DIRECT_ERR_DEVICE.  Sums, minima and
// the stats' maximum are order-independent integers: no output depends on the launch shape.
#pragma once
#include "free_comp_math.h"
#include "grid_path_math.h"

namespace fc = ::direct::freecomp;
static_assert(fc::kTile == ::direct::gridpath::kTile, "the components use the grid paths' tiling");
static_assert(fc::kOk == DIRECT_GRID_PATH_OK && fc::kNoPath == DIRECT_GRID_PATH_NO_PATH && fc::kBadEndpoint == DIRECT_GRID_PATH_BAD_ENDPOINT,
              "a pair is judged with the path calls' codes");

constexpr int kCcBlocks = 16384;  // workgroups of the per-voxel kernels at most (grid-stride beyond)

struct CompDev {
  const uint8_t* map;
  const int32_t* d2;   // the stored field; not read without a floor
  int32_t* label;      // parent during the build
  int32_t* size;
  unsigned long long* cnt;  // [0] enterable voxels, [1] components, [2] stat_key of the largest, [3] the error word
  int X, Y, Z, G, min_d2;
  int tx, ty, tz;
};

struct ReachDev {
  const int32_t *starts, *goals;  // [n][3]
  const int32_t *label, *size;
  int32_t *rtn, *goal_label, *goal_size;  // [n], any may be null
  long long n;
  int X, Y, Z;
};

__device__ __forceinline__ void cc_report(const CompDev& A, int err) {
  if (err) atomicOr((unsigned int*)(A.cnt + 3), (unsigned int)err);
}

__global__ __launch_bounds__(256) void k_cc_tile(CompDev A) {
  __shared__ int s_par[fc::kTileVox];
  const int t = blockIdx.x;
  const int x0 = (t / (A.ty * A.tz)) * fc::kTile, y0 = ((t / A.tz) % A.ty) * fc::kTile, z0 = (t % A.tz) * fc::kTile;
  for (int l = threadIdx.x; l < fc::kTileVox; l += 256) {
    const int x = x0 + (l >> 6), y = y0 + ((l >> 3) & 7), z = z0 + (l & 7);
    int p = -1;
    if (x < A.X && y < A.Y && z < A.Z && fc::enterable(A.map, A.d2, ((long long)x * A.Y + y) * A.Z + z, A.min_d2)) p = l;
    s_par[l] = p;
  }
  __syncthreads();
  auto load = [&](int i) { return __hip_atomic_load(&s_par[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  auto amin = [&](int i, int v) { return __hip_atomic_fetch_min(&s_par[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  int err = 0;
  for (int l = threadIdx.x; l < fc::kTileVox; l += 256) {
    if (load(l) < 0) continue;
    const int lx = l >> 6, ly = (l >> 3) & 7, lz = l & 7;
    for (int k = 0; k < fc::kForward; k++) {
      int dx, dy, dz;
      fc::forward_offset(k, dx, dy, dz);
      const int nx = lx + dx, ny = ly + dy, nz = lz + dz;
      if (nx >= fc::kTile || ny < 0 || ny >= fc::kTile || nz < 0 || nz >= fc::kTile) continue;  // another tile: k_cc_merge
      const int m = (nx << 6) | (ny << 3) | nz;
      if (load(m) < 0) continue;  // outside the map, or not enterable
      fc::unite(load, amin, l, m, fc::kTileVox, &err);
    }
  }
  __syncthreads();
  for (int l = threadIdx.x; l < fc::kTileVox; l += 256) {
    const int x = x0 + (l >> 6), y = y0 + ((l >> 3) & 7), z = z0 + (l & 7);
    if (x >= A.X || y >= A.Y || z >= A.Z) continue;
    int r = -1;
    if (s_par[l] >= 0) {
      const int q = fc::root_of([&](int i) { return s_par[i]; }, l, fc::kTileVox, &err);
      r = ((x0 + (q >> 6)) * A.Y + (y0 + ((q >> 3) & 7))) * A.Z + (z0 + (q & 7));
    }
    A.label[((long long)x * A.Y + y) * A.Z + z] = r;
  }
  cc_report(A, err);
}

__global__ __launch_bounds__(256) void k_cc_merge(CompDev A) {
  auto load = [&](int i) { return __hip_atomic_load(&A.label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto amin = [&](int i, int v) { return __hip_atomic_fetch_min(&A.label[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  const int YZ = A.Y * A.Z;
  int err = 0;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < A.G; g += (long long)gridDim.x * 256) {
    const int v = (int)g;
    const int x = v / YZ, y = (v / A.Z) % A.Y, z = v % A.Z;
    const int lx = x & 7, ly = y & 7, lz = z & 7;
    if (lx != 7 && ly != 0 && ly != 7 && lz != 0 && lz != 7) continue;  // no forward neighbour in another tile
    if (load(v) < 0) continue;
    for (int k = 0; k < fc::kForward; k++) {
      int dx, dy, dz;
      fc::forward_offset(k, dx, dy, dz);
      const int nx = x + dx, ny = y + dy, nz = z + dz;
      if (nx >= A.X || ny < 0 || ny >= A.Y || nz < 0 || nz >= A.Z) continue;
      if ((nx >> 3) == (x >> 3) && (ny >> 3) == (y >> 3) && (nz >> 3) == (z >> 3)) continue;  // the same tile: k_cc_tile
      const int m = (nx * A.Y + ny) * A.Z + nz;
      if (load(m) < 0) continue;
      fc::unite(load, amin, v, m, A.G, &err);
    }
  }
  cc_report(A, err);
}

__global__ __launch_bounds__(256) void k_cc_flatten(CompDev A) {
  auto load = [&](int i) { return __hip_atomic_load(&A.label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  int err = 0;
  const int lane = threadIdx.x & 63;
  // the trip count is the wave's, not the lane's: the lanes of a wave count their roots together below
  for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); base < A.G; base += (long long)gridDim.x * 256) {
    const long long g = base + lane;
    int r = -1;
    if (g < A.G && load((int)g) >= 0) {
      r = fc::root_of(load, (int)g, A.G, &err);
      __hip_atomic_store(&A.label[g], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // one add per distinct root of the wave (neighbouring voxels mostly share theirs), not one per voxel on one word
    unsigned long long todo = __ballot(r >= 0);
    for (int turn = 0; turn < 64 && todo; turn++) {
      const int lead = __ffsll((long long)todo) - 1;
      const int r0 = __shfl(r, lead);
      const unsigned long long same = __ballot(r == r0) & todo;
      if (lane == lead) atomicAdd(&A.size[r0], __popcll(same));
      todo &= ~same;
    }
  }
  cc_report(A, err);
}

__global__ __launch_bounds__(256) void k_cc_sizes(CompDev A) {
  unsigned long long ent = 0, comps = 0, best = 0;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < A.G; g += (long long)gridDim.x * 256) {
    const int r = A.label[g];
    if (r < 0) continue;  // size[g] is 0 from the clear
    ent++;
    if (r != (int)g) {
      A.size[g] = A.size[r];  // a root's word, which no lane writes in this kernel
      continue;
    }
    comps++;
    const unsigned long long key = fc::stat_key(A.size[g], r);
    best = key > best ? key : best;
  }
  for (int o = 32; o > 0; o >>= 1) {
    ent += __shfl_xor(ent, o);
    comps += __shfl_xor(comps, o);
    const unsigned long long other = __shfl_xor(best, o);
    best = other > best ? other : best;
  }
  if ((threadIdx.x & 63) == 0 && ent) {
    atomicAdd(A.cnt, ent);
    if (comps) atomicAdd(A.cnt + 1, comps);
    if (best) atomicMax(A.cnt + 2, best);
  }
}

__global__ __launch_bounds__(256) void k_reach(ReachDev R) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < R.n; i += (long long)gridDim.x * 256) {
    const int32_t s[3] = {R.starts[3 * i], R.starts[3 * i + 1], R.starts[3 * i + 2]};
    const int32_t g[3] = {R.goals[3 * i], R.goals[3 * i + 1], R.goals[3 * i + 2]};
    int32_t gl;
    const int code = fc::reach_pair(s, g, R.X, R.Y, R.Z, [&](int v) { return R.label[v]; }, &gl);
    if (R.rtn) R.rtn[i] = code;
    if (R.goal_label) R.goal_label[i] = gl;
    if (R.goal_size) R.goal_size[i] = gl >= 0 ? R.size[(g[0] * R.Y + g[1]) * R.Z + g[2]] : 0;
  }
}

// Enqueues the build; cnt and size have been cleared on the same stream.
inline hipError_t free_comp_launch(const CompDev& A, hipStream_t stream) {
  const int blocks = (int)std::min<long long>(((long long)A.G + 255) / 256, kCcBlocks);
  hipLaunchKernelGGL(k_cc_tile, dim3(A.tx * A.ty * A.tz), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(k_cc_merge, dim3(blocks), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(k_cc_flatten, dim3(blocks), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(k_cc_sizes, dim3(blocks), dim3(256), 0, stream, A);
  return hipGetLastError();
}
