// Kernels of direct_cluster_distance_field (include/direct_cluster.h, "distance field of the resident map"); included by
// direct_cluster.hip inside its anonymous namespace.  The arithmetic is dist_field_math.h's, shared with the CPU tests.
//
//   k_df_z     one workgroup per run of `ncol` columns, which are contiguous in the map: the run's bytes are copied into LDS with
//              coalesced loads, thread t < ncol sweeps column t up and down in LDS (an int row of odd stride per column, so that
//              the lanes of a wave fall into different banks), and the workgroup writes the run's ints out coalesced.  Without the
//              staging the 64 lanes of a wave would each stride max_z bytes.
//   k_df_scan  passes y and x: one thread per OUTPUT voxel, adjacent lanes adjacent entries of the flattened index, so every load
//              of in[j] is coalesced across the wave (z is contiguous in pass y, the flattened (y, z) in pass x).  The outward
//              scan of distfield::scan_min ends after about the distance itself, and neighbouring lanes have similar distances.
//              The last pass also counts the statistics when they are asked for: one wave reduction, then one atomic add and one
//              atomic max per wave on two counters of their own.
// No persistent kernel, no spin wait, no atomic on the field; every loop is bounded by a dimension or strides over an array.
#pragma once
#include "dist_field_math.h"

namespace df = direct::distfield;

constexpr int kDfTile = 4608;       // ints (and bytes) of LDS a run of columns may fill: 4 columns at max_z = 1024
constexpr int kDfScanBlocks = 8192; // workgroups of k_df_scan at most (grid-stride beyond)

struct DistDev {
  const uint8_t* map;
  int32_t *a, *b;                   // the two field buffers; the finished field is in a
  int X, Y, Z, G, cap2;
  unsigned long long* cnt;          // [0] voxels below cap2, [1] (as int) the largest value below cap2
};

__global__ __launch_bounds__(256) void k_df_z(DistDev A, int ncol) {
  __shared__ int s_out[kDfTile];
  __shared__ uint8_t s_map[kDfTile];
  const int Z = A.Z, zp = Z | 1, ncols = A.X * A.Y;
  const int c0 = blockIdx.x * ncol;
  const int nc = ncols - c0 < ncol ? ncols - c0 : ncol;  // > 0 by the grid's size
  const int bytes = nc * Z;
  const uint8_t* src = A.map + (size_t)c0 * Z;
  for (int q = threadIdx.x; q < bytes; q += 256) s_map[q] = src[q];
  __syncthreads();
  if ((int)threadIdx.x < nc) df::pass_z(s_map + threadIdx.x * Z, 1, Z, A.cap2, s_out + threadIdx.x * zp, 1);
  __syncthreads();
  int32_t* dst = A.a + (size_t)c0 * Z;
  for (int q = threadIdx.x; q < bytes; q += 256) {
    const int c = q / Z;
    dst[q] = s_out[c * zp + (q - c * Z)];
  }
}

// out[g] = min over the line through g along the axis of stride s and length n; `count`: the statistics of out
__global__ __launch_bounds__(256) void k_df_scan(DistDev A, const int32_t* __restrict__ in, int32_t* __restrict__ out, int s, int n,
                                                 int count) {
  long long below = 0;
  int top = -1;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < A.G; g += (long long)gridDim.x * 256) {
    const int i = (int)((g / s) % n);
    const int v = df::scan_min(in + (g - (long long)i * s), (long long)s, n, i);
    out[g] = v;
    if (v < A.cap2) {
      below++;
      top = v > top ? v : top;
    }
  }
  if (!count) return;  // uniform
  for (int o = 32; o > 0; o >>= 1) {
    below += __shfl_xor(below, o);
    const int other = __shfl_xor(top, o);
    top = other > top ? other : top;
  }
  if ((threadIdx.x & 63) == 0 && below) {
    atomicAdd(A.cnt, (unsigned long long)below);
    atomicMax((int*)(A.cnt + 1), top);
  }
}

// Enqueues the three passes; the counters have been set on the same stream (cnt[0] = 0, the int behind cnt[1] = -1).
inline hipError_t dist_field_launch(const DistDev& A, int count, hipStream_t stream) {
  const int zp = A.Z | 1, ncols = A.X * A.Y;
  const int ncol = std::min(256, kDfTile / zp);
  hipLaunchKernelGGL(k_df_z, dim3((ncols + ncol - 1) / ncol), dim3(256), 0, stream, A, ncol);
  const int blocks = (int)std::min<long long>(((long long)A.G + 255) / 256, kDfScanBlocks);
  hipLaunchKernelGGL(k_df_scan, dim3(blocks), dim3(256), 0, stream, A, A.a, A.b, A.Z, A.Y, 0);
  hipLaunchKernelGGL(k_df_scan, dim3(blocks), dim3(256), 0, stream, A, A.b, A.a, A.Y * A.Z, A.X, count);
  return hipGetLastError();
}
