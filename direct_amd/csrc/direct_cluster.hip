// Corridor-cluster generation on gfx950 (include/direct_cluster.h).
//
// Replaces cudaPolytopeGeneration::polygonGeneration of the reference's SHIPPED CPU build
// (polyhedron_generator/src/cluster_server_cpu.cpp:394-528, "CS") for a batch of seed voxels, bit for bit:
//   cubeInflation_cpu    CS:257-293  -> k_inflate   (one workgroup per seed runs ALL rounds and directions on the
//                                       device; the reference's CUDA twin paraCubeInflation, cluster_engine.cu:185-350,
//                                       pays one H2D + launch + D2H per direction per round and reduces through a
//                                       racy single bool; here a face is reduced with __syncthreads_or)
//   getVoxelsInCube + surface extraction CS:62-81, 441-506 -> k_inflate (ordered block-scan compaction)
//   candidate generation CS:301-353  -> k_mark + k_compact (first-discoverer order reproduced with an atomicMin
//                                       of the discovery key per voxel, then an ordered compaction)
//   serialConvexTest     cluster_engine_cpu.cpp:31-136 -> k_convex (one workgroup per candidate, one lane per
//                                       target ray; float DDA exactly as the reference's; a candidate blocked by a
//                                       cluster voxel stops at once)
//   the sequential accept loop CS:360-384 -> k_resolve (one wave; bit-matrix of candidate-candidate rays, the
//                                       device form of paraResultCheck's packed triangle, cluster_engine.cu:37-67)
// Not in the reference: a ray whose axis-aligned box holds no obstacle cannot be blocked (summed-area table of the map,
// k_sat_*; per ray and per chunk of 256 cluster voxels, k_chunk_box) - the results are the reference's, most walks are not run.
// Integer / byte work, HBM- and L2-bound: no MFMA anywhere.  Flag bytes of a seed's grid: bit0 use_data,
// bit1 invalid_data, bit2 inside_data, bit3 map_data == 1 (one load per DDA step instead of two).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/direct_cluster.h"
#include "cluster_corridor_math.h"
#include "cube_corridor_clear_math.h"
#include "cube_corridor_math.h"
#include "free_comp_math.h"
#include "frontier_math.h"
#include "grid_path_clear_math.h"
#include "grid_path_fan_math.h"
#include "grid_path_math.h"
#include "host_stage.h"
#include "hull_core.h"
#include "resident_state.h"

namespace {
namespace rs = ::direct::resident;

constexpr uint8_t F_USE = 1, F_INVALID = 2, F_INSIDE = 4, F_OBS = 8;
constexpr int KEY_NONE = 0x7f7f7f7f;
constexpr int kDimLimit = 1024;  // voxels are packed as x << 20 | y << 10 | z

__device__ __forceinline__ int pack3(int x, int y, int z) { return (x << 20) | (y << 10) | z; }
__device__ __forceinline__ int px(int p) { return p >> 20; }
__device__ __forceinline__ int py(int p) { return (p >> 10) & 1023; }
__device__ __forceinline__ int pz(int p) { return p & 1023; }

struct Elem {  // per-seed counters, device resident
  int n_cluster, n_active, n_cand, iters, live, rtn, pad0, pad1;
  int vertex[24];
};

constexpr int kCompactBlocks = 64;  // workgroups per seed of the candidate compaction
struct Dev {
  int max_x, max_y, max_z, max_yz, G;
  int ccap, kcap, kwords;  // cluster / candidate capacity, 64-bit words per candidate row
  const uint8_t* map;      // [G]
  int* sat;                // [(max_x + 1)(max_y + 1)(max_z + 1)] obstacles in [0, x) x [0, y) x [0, z): summed-area table of map == 1
  int sat_yz, sat_z;       // its strides
  const float* inv;        // [kDimLimit] (float)(1.0 / (double)d), inv[0] = 0: the DDA's tDelta per |d| (ray_walk_lin)
  int* cbox;               // [batch][nchunk][6] bounding box (lo xyz, hi xyz) of every 256 consecutive cluster voxels
  int nchunk;              // (ccap + 255) / 256
  uint8_t* flags;          // [batch][G]
  int* key;                // [batch][G]
  int *cluster, *active;   // [batch][ccap] packed voxels
  int* cand;               // [batch][kcap]
  uint8_t *can_clu, *accept;        // [batch][kcap]
  unsigned long long* blocked;      // [batch][kcap][kwords]
  unsigned long long* accbits;      // [batch][kwords] accepted candidates of the round (k_resolve_fast -> k_apply)
  int* accpre;                      // [batch][kwords] accepted candidates before word w
  Elem* el;                // [batch]
  int* ccnt;               // [batch][kCompactBlocks] first-discoverer counts of k_compact_count's ranges
  int* csnap;              // [batch][2] (live, n_active * 26) as the round's candidate generation saw them
};

// ---- flags <- map ---------------------------------------------------------------------------------------
__global__ void k_flags_init(Dev D, const uint8_t* inside /* or null */) {
  const size_t e = blockIdx.y;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)D.G; i += (size_t)gridDim.x * blockDim.x) {
    uint8_t f = D.map[i] == 1 ? F_OBS : 0;
    if (inside && inside[i] == 1) f |= F_INSIDE;
    D.flags[e * D.G + i] = f;
    D.key[e * D.G + i] = KEY_NONE;
  }
}

// ---- summed-area table of the obstacles (once per map) ----------------------------------------------------
// A ray's walk only visits voxels of the axis-aligned box spanned by its two ends (every axis makes exactly |d| steps,
// see ray_walk_t), and it reports "blocked" only at a voxel with map == 1: a ray whose box holds no obstacle is clear
// whatever else happens on the way.  In free space that is 85 - 97 % of the rays that pass the two cheap tests, and a
// box sum is eight loads against ~25 dependent steps.
__global__ void k_sat_fill(Dev D) {
  const int n = (D.max_x + 1) * D.sat_yz;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int x = i / D.sat_yz, r = i - x * D.sat_yz, y = r / D.sat_z, z = r - y * D.sat_z;
    D.sat[i] = (x > 0 && y > 0 && z > 0 && D.map[(x - 1) * D.max_yz + (y - 1) * D.max_z + (z - 1)] == 1) ? 1 : 0;
  }
}
__global__ void k_sat_scan(Dev D, int axis) {  // running sums along one axis, one thread per line
  const int nx = D.max_x + 1, ny = D.max_y + 1, nz = D.max_z + 1;
  const int lines = axis == 0 ? ny * nz : (axis == 1 ? nx * nz : nx * ny);
  const int len = axis == 0 ? nx : (axis == 1 ? ny : nz);
  const int stride = axis == 0 ? D.sat_yz : (axis == 1 ? D.sat_z : 1);
  for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < lines; l += gridDim.x * blockDim.x) {
    int base;
    if (axis == 0) base = l;                                          // (y, z)
    else if (axis == 1) base = (l / nz) * D.sat_yz + (l % nz);        // (x, z)
    else base = l * nz;                                               // (x, y)
    int acc = 0;
    for (int k = 0; k < len; k++) {
      acc += D.sat[base + k * stride];
      D.sat[base + k * stride] = acc;
    }
  }
}
// obstacles in the box [lo, hi] (inclusive voxel coordinates)
__device__ __forceinline__ int box_obstacles(const Dev& D, int x0, int y0, int z0, int x1, int y1, int z1) {
  // unsigned BYTE offsets from the table's (wave-uniform) base: one 32-bit add per corner, no 64-bit address arithmetic
  const char* S = (const char*)D.sat;
  const unsigned a0 = (unsigned)(x0 * D.sat_yz) << 2, a1 = (unsigned)((x1 + 1) * D.sat_yz) << 2, b0 = (unsigned)(y0 * D.sat_z) << 2,
                 b1 = (unsigned)((y1 + 1) * D.sat_z) << 2, c0 = (unsigned)z0 << 2, c1 = (unsigned)(z1 + 1) << 2;
  auto at = [&](unsigned off) { return *(const int*)(S + off); };
  const unsigned a0b0 = a0 + b0, a0b1 = a0 + b1, a1b0 = a1 + b0, a1b1 = a1 + b1;
  return at(a1b1 + c1) - at(a0b1 + c1) - at(a1b0 + c1) - at(a1b1 + c0) + at(a0b0 + c1) + at(a0b1 + c0) + at(a1b0 + c0) - at(a0b0 + c0);
}

// exclusive position of `flag` among the flags of a 256-thread block + the block total (ordered compaction)
__device__ __forceinline__ int block_scan256(int flag, int* total, int* wsum /* shared[4] */) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pos = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
  for (int q = 0; q < 4; q++) {
    if (q < w) base += wsum[q];
    tot += wsum[q];
  }
  *total = tot;
  return base + pos;
}

// ---- cube inflation + initial surface cluster (CS:257-293, 400-518) ---------------------------------------
__global__ __launch_bounds__(256) void k_inflate(Dev D, const int* seeds, int itr_inflate_max) {
  __shared__ int v[24], vl[24], wsum[4];
  const int e = blockIdx.x, tid = threadIdx.x;
  Elem* E = &D.el[e];
  uint8_t* fl = D.flags + (size_t)e * D.G;
  const int sx = seeds[3 * e], sy = seeds[3 * e + 1], sz = seeds[3 * e + 2];
  if (sx < 0 || sx >= D.max_x || sy < 0 || sy >= D.max_y || sz < 0 || sz >= D.max_z) {
    if (tid == 0) {
      E->n_cluster = E->n_active = E->n_cand = E->iters = E->live = 0;
      E->rtn = DIRECT_CLUSTER_BAD_SEED;
      for (int q = 0; q < 24; q++) E->vertex[q] = 0;
    }
    return;
  }
  if (tid < 8) { v[tid] = vl[tid] = sx; v[tid + 8] = vl[tid + 8] = sy; v[tid + 16] = vl[tid + 16] = sz; }  // CS:400-408
  __syncthreads();
  const int step = 1;  // inf_step, CS:117
  for (int iter = 0; iter < itr_inflate_max; iter++) {
    for (int dir = 0; dir < 6; dir++) {  // Y-, Y+, X-, X+, Z-, Z+ (CS:263-268)
      // the face slab one voxel beyond the cube: ranges (a, b) and the fixed coordinate, per CS:126-255
      int a0, a1, b0, b1, fixed, edge;
      switch (dir) {
        case 0: edge = v[8] == 0;            fixed = v[8] - 1;  a0 = v[3]; a1 = v[0]; b0 = v[20]; b1 = v[16]; break;
        case 1: edge = v[9] == D.max_y - 1;  fixed = v[9] + 1;  a0 = v[2]; a1 = v[1]; b0 = v[21]; b1 = v[17]; break;
        case 2: edge = v[3] == 0;            fixed = v[3] - 1;  a0 = v[11]; a1 = v[10]; b0 = v[23]; b1 = v[19]; break;
        case 3: edge = v[0] == D.max_x - 1;  fixed = v[0] + 1;  a0 = v[8]; a1 = v[9]; b0 = v[20]; b1 = v[16]; break;
        case 4: edge = v[20] == 0;           fixed = v[20] - 1; a0 = v[7]; a1 = v[4]; b0 = v[12]; b1 = v[13]; break;
        default: edge = v[16] == D.max_z - 1; fixed = v[16] + 1; a0 = v[3]; a1 = v[0]; b0 = v[8]; b1 = v[9]; break;
      }
      int hit = 0;
      if (!edge) {
        const int nb = b1 - b0 + 1, cells = (a1 - a0 + 1) * nb;
        for (int c = tid; c < cells; c += 256) {
          const int a = a0 + c / nb, b = b0 + c % nb;
          int id;
          if (dir < 2) id = a * D.max_yz + fixed * D.max_z + b;        // (x, fixed y, z)
          else if (dir < 4) id = fixed * D.max_yz + a * D.max_z + b;   // (fixed x, y, z)
          else id = a * D.max_yz + b * D.max_z + fixed;                // (x, y, fixed z)
          hit |= D.map[id] > 0;
        }
      }
      const int blocked = __syncthreads_or(hit);
      if (tid == 0 && !edge && !blocked) {
        switch (dir) {
          case 0: v[8] -= step; v[11] -= step; v[12] -= step; v[15] -= step; break;
          case 1: v[9] += step; v[10] += step; v[13] += step; v[14] += step; break;
          case 2: v[2] -= step; v[3] -= step; v[6] -= step; v[7] -= step; break;
          case 3: v[0] += step; v[1] += step; v[4] += step; v[5] += step; break;
          case 4: v[20] -= step; v[21] -= step; v[22] -= step; v[23] -= step; break;
          default: v[16] += step; v[17] += step; v[18] += step; v[19] += step; break;
        }
      }
      __syncthreads();
    }
    const int changed = __syncthreads_or(tid < 24 ? (v[tid] != vl[tid]) : 0);  // CS:270-281
    if (!changed) break;
    if (tid < 24) vl[tid] = v[tid];
    __syncthreads();
  }
  if (tid < 24) E->vertex[tid] = v[tid];
  // getVoxelsInCube (CS:62-81) and the surface cells (CS:441-489), in x, y, z order
  const int x0 = v[7], x1 = v[1], y0 = v[15], y1 = v[9], z0 = v[23], z1 = v[17];
  const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, nz = z1 - z0 + 1;
  const long ncube = (long)nx * ny * nz;
  int* cl = D.cluster + (size_t)e * D.ccap;
  int* ac = D.active + (size_t)e * D.ccap;
  int n_out = 0, overflow = 0;
  if (ncube == 1) {  // CS:433-439: the cell is its own surface; use_data is NOT set on this branch
    if (tid == 0) cl[0] = ac[0] = pack3(x0, y0, z0);
    n_out = 1;
  } else {
    for (long base = 0; base < ncube; base += 256) {
      const long c = base + tid;
      int surf = 0, p = 0;
      if (c < ncube) {
        const int x = x0 + (int)(c / ((long)ny * nz)), r = (int)(c % ((long)ny * nz)), y = y0 + r / nz, z = z0 + r % nz;
        p = pack3(x, y, z);
        // a cell is interior iff all 26 neighbours lie in the cube (and hence in the map): strictly inside the box
        surf = x == x0 || x == x1 || y == y0 || y == y1 || z == z0 || z == z1;
        const int id = x * D.max_yz + y * D.max_z + z;
        fl[id] = (fl[id] & F_OBS) | F_USE | (surf ? 0 : F_INSIDE);  // CS:447, 76, 491-494
      }
      int tot;
      const int pos = block_scan256(surf, &tot, wsum);
      if (surf) {
        if (n_out + pos < D.ccap) cl[n_out + pos] = ac[n_out + pos] = p;
        else overflow = 1;
      }
      n_out += tot;
      __syncthreads();
    }
  }
  overflow = __syncthreads_or(overflow);
  if (tid == 0) {
    const int degenerate = x0 == x1 || y0 == y1 || z0 == z1;  // CS:509-518
    E->n_cluster = E->n_active = overflow ? D.ccap : n_out;
    E->n_cand = 0;
    E->iters = 0;
    E->rtn = overflow ? DIRECT_CLUSTER_OVERFLOW : DIRECT_CLUSTER_OK;
    E->live = (!overflow && !degenerate) ? 1 : 0;
  }
}

// ---- candidate generation (CS:301-353) -------------------------------------------------------------------
// discovery key of (active voxel a, neighbour n): the order in which the sequential loop would reach it
__device__ __forceinline__ int neighbour_id(const Dev& D, int p, int n, int* packed) {
  const int q = n < 13 ? n : n + 1;  // 27 offsets without the centre, dx outermost (CS:315-319)
  const int x = px(p) + q / 9 - 1, y = py(p) + (q / 3) % 3 - 1, z = pz(p) + q % 3 - 1;
  if (x < 0 || x > D.max_x - 1 || y < 0 || y > D.max_y - 1 || z < 0 || z > D.max_z - 1) return -1;
  *packed = pack3(x, y, z);
  return x * D.max_yz + y * D.max_z + z;
}
__global__ void k_mark(Dev D) {
  const int e = blockIdx.y;
  const Elem* E = &D.el[e];
  if (!E->live) return;
  const int total = E->n_active * 26;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {  // grid stride: the launch
                                                                                                 // does not depend on n_active
    int p;
    const int id = neighbour_id(D, D.active[(size_t)e * D.ccap + t / 26], t % 26, &p);
    // map == 1 || use || invalid || inside -> skip (CS:332-338): all four are bits of the one flag byte
    if (id >= 0 && D.flags[(size_t)e * D.G + id] == 0) atomicMin(&D.key[(size_t)e * D.G + id], t);
  }
}
// Ordered compaction of the first discoverers into the candidate list, kCompactBlocks workgroups per seed (one
// workgroup walking all n_active x 26 neighbours was 84 us per round, 8 % of the generation): every workgroup owns a
// contiguous range of the discovery order; k_compact_count counts its first discoverers, k_compact_write places them
// behind those of the ranges before it.  The Elem is only written by k_compact_write's workgroup 0, and nobody in that
// kernel reads it (csnap carries what the round started from).
__device__ __forceinline__ void compact_range(int total, int b, int* lo, int* hi) {
  const int per = (((total + kCompactBlocks - 1) / kCompactBlocks) + 255) & ~255;
  *lo = b * per;
  *hi = *lo + per < total ? *lo + per : total;
}
__global__ __launch_bounds__(256) void k_compact_count(Dev D) {
  __shared__ int wsum[4];
  const int e = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const Elem* E = &D.el[e];
  const int live = E->live, total = live ? E->n_active * 26 : 0;
  if (b == 0 && tid == 0) { D.csnap[2 * e] = live; D.csnap[2 * e + 1] = total; }
  int lo, hi, n = 0;
  compact_range(total, b, &lo, &hi);
  for (int base = lo; base < hi; base += 256) {
    const int t = base + tid;
    int first = 0, p = 0;
    if (t < hi) {
      const int id = neighbour_id(D, D.active[(size_t)e * D.ccap + t / 26], t % 26, &p);
      first = id >= 0 && D.key[(size_t)e * D.G + id] == t;
    }
    n += __popcll(__ballot(first));
  }
  if ((tid & 63) == 0) wsum[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) D.ccnt[e * kCompactBlocks + b] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__global__ __launch_bounds__(256) void k_compact_write(Dev D) {
  __shared__ int wsum[4];
  __shared__ int s_off, s_all;
  const int e = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  if (!D.csnap[2 * e]) return;
  const int total = D.csnap[2 * e + 1];
  if (tid < 64) {  // kCompactBlocks == 64: one count per lane
    const int c = D.ccnt[e * kCompactBlocks + tid];
    int before = tid < b ? c : 0, all = c;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { before += __shfl_xor(before, d); all += __shfl_xor(all, d); }
    if (tid == 0) { s_off = before; s_all = all; }
  }
  __syncthreads();
  int n_out = s_off;
  const int all = s_all;
  int lo, hi;
  compact_range(total, b, &lo, &hi);
  for (int base = lo; base < hi; base += 256) {
    const int t = base + tid;
    int first = 0, p = 0, id = -1;
    if (t < hi) {
      id = neighbour_id(D, D.active[(size_t)e * D.ccap + t / 26], t % 26, &p);
      first = id >= 0 && D.key[(size_t)e * D.G + id] == t;
    }
    int tot;
    const int pos = block_scan256(first, &tot, wsum);
    if (first) {
      D.key[(size_t)e * D.G + id] = KEY_NONE;
      D.flags[(size_t)e * D.G + id] |= F_USE;  // CS:347
      if (n_out + pos < D.kcap) D.cand[(size_t)e * D.kcap + n_out + pos] = p;
    }
    n_out += tot;
    __syncthreads();
  }
  if (b == 0 && tid == 0) {
    Elem* E = &D.el[e];
    const int overflow = all > D.kcap;
    E->n_cand = overflow ? 0 : all;
    if (overflow) { E->rtn = DIRECT_CLUSTER_OVERFLOW; E->live = 0; }
    else if (all == 0) E->live = 0;  // CS:356-357
  }
}

// ---- serialConvexTest, one ray (cluster_engine_cpu.cpp:44-131).  Returns 1 when an obstacle blocks it. -------
__device__ __forceinline__ float intbound_half(int ds) {
  // intbound_cpu(0.5, ds), cluster_engine_cpu.cpp:13-29: mod(+-0.5, 1) is 0.5 for either sign, so the value is
  // 0.5f / |ds| in float; computed in double and rounded once, which is the correctly rounded float quotient
  if (ds == 0) return INFINITY;  // numeric_limits<double>::max() returned through float
  return (float)(0.5 / (double)(ds < 0 ? -ds : ds));
}
// RD(x, y, z) -> flag byte of a voxel (only F_INSIDE and F_OBS are looked at)
// the two cheap tests in front of the walk: 1 when the ray has to be traced
template <typename RD>
__device__ __forceinline__ int ray_needs_walk_t(const RD& rd, int cx, int cy, int cz, int target) {
  const int ex = px(target), ey = py(target), ez = pz(target);
  if (rd(ex, ey, ez) & F_INSIDE) return 0;  // only targets with inside_data == 0 are traced
  const int mx = cx / 2 + (ex >> 1), my = cy / 2 + (ey >> 1), mz = cz / 2 + (ez >> 1);
  if (rd(mx, my, mz) & F_INSIDE) return 0;  // "midpoint" inside the cube: skipped
  return 1;
}
template <typename RD>
__device__ __forceinline__ int ray_walk_t(const RD& rd, int cx, int cy, int cz, int target);
template <typename RD>
__device__ __forceinline__ int ray_blocked_t(const RD& rd, int cx, int cy, int cz, int target) {
  return ray_needs_walk_t(rd, cx, cy, cz, target) ? ray_walk_t(rd, cx, cy, cz, target) : 0;
}
template <typename RD>
__device__ __forceinline__ int ray_walk_t(const RD& rd, int cx, int cy, int cz, int target) {
  const int ex = px(target), ey = py(target), ez = pz(target);
  int x = cx, y = cy, z = cz;
  const int dx = ex - x, dy = ey - y, dz = ez - z;
  const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0), sz = (dz > 0) - (dz < 0);
  float tMaxX = intbound_half(dx), tMaxY = intbound_half(dy), tMaxZ = intbound_half(dz);
  // tDelta = ((float)step) / d: 1 / |d| correctly rounded, NaN (0 / 0) for d == 0 - never added: tMax stays +inf
  const float tDX = dx ? (float)(1.0 / (double)(dx < 0 ? -dx : dx)) : 0.0f;
  const float tDY = dy ? (float)(1.0 / (double)(dy < 0 ? -dy : dy)) : 0.0f;
  const float tDZ = dz ? (float)(1.0 / (double)(dz < 0 ? -dz : dz)) : 0.0f;
  int budget = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
  for (;;) {
    if (tMaxX < tMaxY) {
      if (tMaxX < tMaxZ) { x += sx; tMaxX += tDX; }
      else               { z += sz; tMaxZ += tDZ; }
    } else {
      if (tMaxY < tMaxZ) { y += sy; tMaxY += tDY; }
      else               { z += sz; tMaxZ += tDZ; }
    }
    if (x == ex && y == ey && z == ez) return 0;
    // each axis makes exactly |d| steps before the end voxel is reached; a ray that float rounding made miss its
    // end would leave the map (the reference then reads outside its arrays): cut off, reported as clear
    if (--budget < 0) return 0;
    const unsigned f = rd(x, y, z);
    if (f & F_INSIDE) return 0;
    if (f & F_OBS) return 1;
  }
}
// The walk as k_convex runs it - the same float sequence, cheaper around it: 1 / |d| from a table (built once per handle
// by the double division above; intbound_half(d) = 0.5 / |d| is exactly half of it: tested for every |d| < 2048), ONE
// linear voxel index that moves by the axis' stride (a voxel has one index, so "end reached" is one compare; no axis makes
// more than |d| steps before the end is reached - the tMax of a finished axis is above 1, those of the others below - so
// the index never leaves the box of the two ends and cannot alias another voxel's).
__global__ void k_inv_table(float* inv) {
  for (int d = threadIdx.x; d < kDimLimit; d += blockDim.x) inv[d] = d ? (float)(1.0 / (double)d) : 0.0f;
}
__device__ __forceinline__ int ray_walk_lin(const Dev& D, const uint8_t* fl, const float* inv, int cx, int cy, int cz, int target) {
  const int dx = px(target) - cx, dy = py(target) - cy, dz = pz(target) - cz;
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
  const int ix = dx < 0 ? -D.max_yz : D.max_yz, iy = dy < 0 ? -D.max_z : D.max_z, iz = dz < 0 ? -1 : 1;  // never taken for d == 0
  const float tDX = inv[ax], tDY = inv[ay], tDZ = inv[az];
  float tMaxX = dx ? 0.5f * tDX : INFINITY, tMaxY = dy ? 0.5f * tDY : INFINITY, tMaxZ = dz ? 0.5f * tDZ : INFINITY;
  int id = cx * D.max_yz + cy * D.max_z + cz;
  const int eid = px(target) * D.max_yz + py(target) * D.max_z + pz(target);
  int budget = ax + ay + az;
  for (;;) {
    if (tMaxX < tMaxY) {
      if (tMaxX < tMaxZ) { id += ix; tMaxX += tDX; }
      else               { id += iz; tMaxZ += tDZ; }
    } else {
      if (tMaxY < tMaxZ) { id += iy; tMaxY += tDY; }
      else               { id += iz; tMaxZ += tDZ; }
    }
    if (id == eid) return 0;
    if (--budget < 0) return 0;
    const unsigned f = fl[id];
    if (f & F_INSIDE) return 0;
    if (f & F_OBS) return 1;
  }
}
// The same walk with the loads taken off its critical path.  Which voxel comes next never depends on what the voxels
// hold - only WHEN the walk ends does - so a trip of the loop advances kWalkDepth voxels (selects, no branch: a lane whose
// walk has reached its end voxel or used up its budget stands still on a valid voxel), issues their loads together and then
// judges them in step order; steps taken past a hit are thrown away.  The loop is uniform over the wave (it runs while any
// lane is undecided), so there is no exec-mask bookkeeping for the four exits of the serial form either.  Same float
// sequence, same visiting order, same answer as ray_walk_lin bit for bit (tests/test_gpu_cluster.py).
#ifndef CLUSTER_WALK_DEPTH
#define CLUSTER_WALK_DEPTH 4
#endif
constexpr int kWalkDepth = CLUSTER_WALK_DEPTH;
__device__ __forceinline__ int ray_walk_pipe(const Dev& D, const uint8_t* fl, const float* inv, int cx, int cy, int cz, int target, int valid) {
  const int tg = valid ? target : 0;
  const int ex = valid ? px(tg) : cx, ey = valid ? py(tg) : cy, ez = valid ? pz(tg) : cz;
  const int dx = ex - cx, dy = ey - cy, dz = ez - cz;
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
  const int ix = dx < 0 ? -D.max_yz : D.max_yz, iy = dy < 0 ? -D.max_z : D.max_z, iz = dz < 0 ? -1 : 1;
  const float tDX = inv[(unsigned)ax], tDY = inv[(unsigned)ay], tDZ = inv[(unsigned)az];
  float tMaxX = dx ? 0.5f * tDX : INFINITY, tMaxY = dy ? 0.5f * tDY : INFINITY, tMaxZ = dz ? 0.5f * tDZ : INFINITY;
  const int cid = cx * D.max_yz + cy * D.max_z + cz;
  int id = cid;
  const int eid = ex * D.max_yz + ey * D.max_z + ez;
  int budget = ax + ay + az;
  int res = valid ? -1 : 0;  // -1: walking
  while (__any(res < 0)) {
    bool live = res < 0;
    unsigned f[kWalkDepth];
    bool lv[kWalkDepth];
#pragma unroll
    for (int u = 0; u < kWalkDepth; u++) {
      const bool xy = tMaxX < tMaxY, xz = tMaxX < tMaxZ, yz = tMaxY < tMaxZ;
      const bool sx = xy & xz, sy = !xy & yz;  // (bitwise on purpose: three lane masks, no selects of booleans)
      const bool sz = !(sx | sy);
      const int nid = id + (sx ? ix : (sy ? iy : iz));
      const float nx = tMaxX + tDX, ny = tMaxY + tDY, nz = tMaxZ + tDZ;
      tMaxX = sx ? nx : tMaxX;  // (what a lane that stands still does to its tMax is never looked at again)
      tMaxY = sy ? ny : tMaxY;
      tMaxZ = sz ? nz : tMaxZ;
      budget -= 1;
      live = live & (nid != eid) & (budget >= 0);
      id = live ? nid : cid;  // a walk that is over stands on the candidate's own voxel: the SAME cache line for every such lane
      lv[u] = live;           // of the wave (k_convex runs at the L1's line rate: a lane parked on a line of its own costs a lookup)
      f[u] = fl[(unsigned)id];  // (a voxel index is never negative: base + 32-bit offset addressing)
    }
    // The four flag bytes side by side, a finished step standing in as "inside" (-> 0): the lowest set bit of the word is the
    // first step that ends the walk, and within a byte F_INSIDE (bit 2) comes before F_OBS (bit 3) as in the serial walk.
    static_assert(kWalkDepth <= 4 && F_INSIDE == 4 && F_OBS == 8, "one byte per step");
    unsigned P = 0;
#pragma unroll
    for (int u = 0; u < kWalkDepth; u++) P |= (lv[u] ? f[u] : (unsigned)F_INSIDE) << (8 * u);
    P &= 0x0c0c0c0cu;
    const int pos = __builtin_ctz(P | 0x80000000u);
    const int r = P == 0u ? -1 : (((pos & 7) == 3) ? 1 : 0);
    res = res >= 0 ? res : r;
  }
  return res;
}
// the tests in front of a walk as k_convex runs them: the reference's two, then the box test
// (any_target: the kernel-level entry point takes arbitrary targets; inside polygonGeneration a target is a cluster voxel or
// a candidate, and neither lies inside the cube: CS:491-494, 301-353)
// Inside polygonGeneration inside_data is the strict interior of the inflated cube and nothing else (k_inflate writes it
// once, CS:441-494; no later kernel touches the bit): the midpoint test is three range compares on the cube's corners instead
// of a scattered byte load per ray - a third of the loads in front of the walks (12 G rays per 64-seed call).  The kernel-level
// entry point (FULL) takes an arbitrary inside_data array and keeps the load.
struct CubeBox {
  int x0, x1, y0, y1, z0, z1;  // inside <=> x0 < x < x1 && y0 < y < y1 && z0 < z < z1
};
template <bool FULL>
__device__ __forceinline__ int ray_needs_walk(const Dev& D, const uint8_t* fl, const CubeBox& cb, int cx, int cy, int cz, int target) {
  const int ex = px(target), ey = py(target), ez = pz(target);
  if (FULL && (fl[(unsigned)(ex * D.max_yz + ey * D.max_z + ez)] & F_INSIDE)) return 0;
  const int mx = cx / 2 + (ex >> 1), my = cy / 2 + (ey >> 1), mz = cz / 2 + (ez >> 1);
  if (FULL) {
    if (fl[(unsigned)(mx * D.max_yz + my * D.max_z + mz)] & F_INSIDE) return 0;
  } else if ((mx > cb.x0) & (mx < cb.x1) & (my > cb.y0) & (my < cb.y1) & (mz > cb.z0) & (mz < cb.z1)) {
    return 0;
  }
  return box_obstacles(D, cx < ex ? cx : ex, cy < ey ? cy : ey, cz < ez ? cz : ez, cx < ex ? ex : cx, cy < ey ? ey : cy,
                       cz < ez ? ez : cz) != 0;
}
__device__ __forceinline__ int ray_blocked(const Dev& D, const uint8_t* fl, int cx, int cy, int cz, int target) {
  return ray_blocked_t([&](int x, int y, int z) -> unsigned { return fl[x * D.max_yz + y * D.max_z + z]; }, cx, cy, cz, target);
}

// bounding boxes of the cluster in chunks of 256 voxels (cluster order is spatially coherent: the cube's surface layer by
// layer, then every round's shell): k_convex tests a candidate against a whole chunk's box before it looks at its rays
__global__ __launch_bounds__(256) void k_chunk_box(Dev D) {
  __shared__ int red[4][6];
  const int e = blockIdx.y, m = blockIdx.x, tid = threadIdx.x;
  const Elem* E = &D.el[e];
  if (!E->live) return;
  const int n = E->n_cluster;
  if (m * 256 >= n) return;
  const int t = m * 256 + tid;
  int v[6] = {kDimLimit, kDimLimit, kDimLimit, -1, -1, -1};
  if (t < n) {
    const int p = D.cluster[(size_t)e * D.ccap + t];
    v[0] = v[3] = px(p); v[1] = v[4] = py(p); v[2] = v[5] = pz(p);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const int lo = __shfl_xor(v[a], d), hi = __shfl_xor(v[a + 3], d);
      v[a] = lo < v[a] ? lo : v[a];
      v[a + 3] = hi > v[a + 3] ? hi : v[a + 3];
    }
  if ((tid & 63) == 0)
    for (int a = 0; a < 6; a++) red[tid >> 6][a] = v[a];
  __syncthreads();
  if (tid < 6) {
    int r = red[0][tid];
    for (int w = 1; w < 4; w++) r = tid < 3 ? (red[w][tid] < r ? red[w][tid] : r) : (red[w][tid] > r ? red[w][tid] : r);
    D.cbox[((size_t)e * D.nchunk + m) * 6 + tid] = r;
  }
}

// one workgroup per candidate.  full = 1 (kernel-level parity entry point): no early exit, every row is complete
template <bool FULL>
__device__ __forceinline__ void convex_one(const Dev& D, const Elem* E, int e, int i);
// A workgroup takes the candidates blockIdx.x, blockIdx.x + gridDim.x, ... of its seed: the grid is sized for the
// typical shell (a few thousand candidates), not for the candidate CAPACITY - one workgroup per capacity slot meant
// 640 k workgroups per round for 64 seeds, nine in ten of which only looked at n_cand and left (44 M wave launches per
// call, ~10 % of the kernel's time).
template <bool FULL>
__global__ __launch_bounds__(256) void k_convex(Dev D) {
  const int e = blockIdx.y;
  const Elem* E = &D.el[e];
  if (!E->live) return;
  const int n_cand = E->n_cand;
  for (int i = blockIdx.x; i < n_cand; i += gridDim.x) {
    convex_one<FULL>(D, E, e, i);
    __syncthreads();  // the next candidate reuses the workgroup's LDS
  }
}
#if defined(CLUSTER_WALK_SERIAL)  // A/B builds: the branching one-voxel-per-trip walk
#define WALK(D, fl, inv, cx, cy, cz, q, valid) ((valid) ? ray_walk_lin(D, fl, inv, cx, cy, cz, q) : 0)
#else
#define WALK ray_walk_pipe
#endif
template <bool FULL>
__device__ __forceinline__ void convex_one(const Dev& D, const Elem* E, int e, int i) {
  constexpr int full = FULL ? 1 : 0;
  const int tid = threadIdx.x;
  // the inflated cube (k_inflate: E->vertex; corner 7 is its low, corner 1 / 9 / 17 its high end per axis)
  CubeBox cb;
  cb.x0 = E->vertex[7]; cb.x1 = E->vertex[1]; cb.y0 = E->vertex[15]; cb.y1 = E->vertex[9]; cb.z0 = E->vertex[23]; cb.z1 = E->vertex[17];
  const uint8_t* fl = D.flags + (size_t)e * D.G;
  const int* cl = D.cluster + (size_t)e * D.ccap;
  const int* cd = D.cand + (size_t)e * D.kcap;
  const int c = cd[i], cx = px(c), cy = py(c), cz = pz(c), n_clu = E->n_cluster;
  int bad = 0;
  // About half of a candidate's rays towards the cluster end at the two cheap tests (the midpoint lies inside the
  // inflated cube) and most of the rest at the box test: left in place they idle through the walks of their wave.  The
  // rays that have to be walked are queued (in order) and walked 64 at a time, every lane busy; the result is an AND, so
  // the order is free.  Every WAVE keeps its own queue and takes every fourth run of 64 targets: no workgroup barrier
  // inside the loops (two per 256 rays cost more than the tests between them), a flag in LDS carries the early exit.
  __shared__ int queue[4][128];
  __shared__ int s_bad;
  __shared__ unsigned char skip[256];
  const float* inv = D.inv;
  const int lane = tid & 63, wv = tid >> 6;
  int* wq = queue[wv];
  int head = 0, count = 0;  // uniform over the wave
  // whole chunks first: a chunk whose box, joined with the candidate, holds no obstacle cannot block it (k_chunk_box)
  const int nch = (n_clu + 255) >> 8;
  if (tid == 0) s_bad = 0;
  if (tid < nch) {
    const int* bx = D.cbox + ((size_t)e * D.nchunk + tid) * 6;
    skip[tid] = box_obstacles(D, cx < bx[0] ? cx : bx[0], cy < bx[1] ? cy : bx[1], cz < bx[2] ? cz : bx[2], cx > bx[3] ? cx : bx[3],
                              cy > bx[4] ? cy : bx[4], cz > bx[5] ? cz : bx[5]) == 0;
  }
  __syncthreads();
  // the wave's ordered append / take: LDS executes a wave's accesses in order, the barrier only stops the compiler
  auto push = [&](int need, int val) {
    const unsigned long long bal = __ballot(need);
    if (need) wq[(head + count + __popcll(bal & ((1ull << lane) - 1ull))) & 127] = val;
    count += __popcll(bal);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto take = [&](int n) {  // the lane's queued value (-1: none)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int v = lane < n ? wq[(head + lane) & 127] : -1;
    head = (head + n) & 127;
    count -= n;
    __builtin_amdgcn_wave_barrier();
    return v;
  };
  for (int m = nch - 1; m >= 0; m--) {
    // newest cluster voxels first, like the reference's loop (cluster_engine_cpu.cpp:41): they lie next to the
    // candidate shell and are the likeliest to reject, so the early exit below comes sooner
    if (m < 256 && skip[m]) continue;
    const int t = m * 256 + tid;
    int tgt = 0, need = 0;
    if (t < n_clu) {
      tgt = cl[t];
      need = ray_needs_walk<FULL>(D, fl, cb, cx, cy, cz, tgt);
    }
    push(need, tgt);
    if (count >= 64) {
      const int q = take(64);
      bad |= WALK(D, fl, inv, cx, cy, cz, q, 1);
      if (!full && __any(bad)) s_bad = 1;  // a rejected candidate's rays towards other candidates are never consulted
    }
    if (!full && *(volatile int*)&s_bad) break;
  }
  if (count > 0 && !(!full && *(volatile int*)&s_bad)) {
    const int q = take(count);
    bad |= WALK(D, fl, inv, cx, cy, cz, q, q >= 0);
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) D.can_clu[(size_t)e * D.kcap + i] = bad ? 0 : 1;
  if (bad && !full) return;
  unsigned long long* row = D.blocked + ((size_t)e * D.kcap + i) * D.kwords;
  constexpr int kRowWords = 256;  // candidate capacities up to 16384 take the queued form
  __shared__ unsigned long long srow[kRowWords];
  if (D.kwords > kRowWords) {
    for (int base = 0; base < i; base += 256) {  // rays towards the candidates before this one
      const int j = base + tid;
      const int b = j < i ? ray_blocked(D, fl, cx, cy, cz, cd[j]) : 0;
      const unsigned long long m = __ballot(b);
      if ((tid & 63) == 0 && base + (tid & ~63) < i) row[(base + tid) >> 6] = m;
    }
    return;
  }
  // the same queues for the rays towards the earlier candidates: the row of the bit matrix is collected in LDS (a blocked
  // ray is rare: one ds_or per hit) and written once
  const int nw = (i + 63) / 64;
  for (int w = tid; w < nw; w += 256) srow[w] = 0ull;
  head = 0;
  count = 0;
  __syncthreads();
  for (int base = 0; base < i; base += 256) {
    const int j = base + tid;
    push(j < i ? ray_needs_walk<FULL>(D, fl, cb, cx, cy, cz, cd[j]) : 0, j);
    if (count >= 64) {
      const int jq = take(64);
      if (WALK(D, fl, inv, cx, cy, cz, cd[jq], 1)) atomicOr(&srow[jq >> 6], 1ull << (jq & 63));
    }
  }
  if (count > 0) {
    const int jq = take(count);
    if (WALK(D, fl, inv, cx, cy, cz, jq >= 0 ? cd[jq] : 0, jq >= 0)) atomicOr(&srow[jq >> 6], 1ull << (jq & 63));
  }
  __syncthreads();
  int nz = 0;
  for (int w = tid; w < nw; w += 256) {
    row[w] = srow[w];
    nz |= srow[w] != 0ull;
  }
  // A candidate that sees the cluster AND every earlier candidate joins whatever the accept loop decides about the
  // others (CS:360-384: it is only ever compared with candidates it cannot see): marked 2, and k_resolve_fast takes it
  // without a place in its sequential chain - which then only holds the few candidates with a blocked ray
  nz = __syncthreads_or(nz);
  if (!full && !nz && tid == 0) D.can_clu[(size_t)e * D.kcap + i] = 2;
}

// the sequential accept loop (CS:360-384) for one seed: one wave.  dry = 1: only accept[] is written.
__global__ __launch_bounds__(64) void k_resolve(Dev D, int dry) {
  extern __shared__ unsigned long long acc[];  // accepted-candidate bitset, kwords words
  const int e = blockIdx.x, lane = threadIdx.x;
  Elem* E = &D.el[e];
  if (!E->live) return;
  const int n_cand = E->n_cand, n_clu = E->n_cluster;
  for (int w = lane; w < D.kwords; w += 64) acc[w] = 0ull;
  __syncthreads();
  int count = 0, overflow = 0;
  const int* cd = D.cand + (size_t)e * D.kcap;
  int* cl = D.cluster + (size_t)e * D.ccap;
  int* ac = D.active + (size_t)e * D.ccap;
  uint8_t* fl = D.flags + (size_t)e * D.G;
  for (int i = 0; i < n_cand; i++) {
    int ok = D.can_clu[(size_t)e * D.kcap + i] != 0;
    if (ok) {
      const unsigned long long* row = D.blocked + ((size_t)e * D.kcap + i) * D.kwords;
      int hit = 0;
      for (int w = lane; w < (i + 63) / 64; w += 64) hit |= (row[w] & acc[w]) != 0ull;
      ok = !__any(hit);
    }
    if (lane == 0) {
      D.accept[(size_t)e * D.kcap + i] = (uint8_t)ok;
      if (ok) acc[i >> 6] |= 1ull << (i & 63);
      if (!dry) {
        const int p = cd[i];
        if (ok) {
          if (n_clu + count < D.ccap) { cl[n_clu + count] = p; ac[count] = p; }
          else overflow = 1;
        } else {
          fl[px(p) * D.max_yz + py(p) * D.max_z + pz(p)] |= F_INVALID;  // CS:380-383
        }
      }
    }
    count += ok;
    __syncthreads();
  }
  if (lane == 0 && !dry) {
    if (overflow) { E->rtn = DIRECT_CLUSTER_OVERFLOW; E->live = 0; E->n_cluster = D.ccap; E->n_active = 0; }
    else {
      E->n_cluster = n_clu + count;
      E->n_active = count;
      if (count == 0) E->live = 0;  // CS:386-387
      else E->iters += 1;           // CS:389
    }
  }
}

// The sequential accept loop (CS:360-384) of one round, one wave per seed, with the candidate's row of the bit matrix
// fetched ONE CANDIDATE AHEAD: the loop is a chain of dependent global loads otherwise (1.5 us per candidate).
__global__ __launch_bounds__(64) void k_resolve_pipe(Dev D) {
  extern __shared__ unsigned long long acc[];  // accepted-candidate bitset, kwords words
  const int e = blockIdx.x, lane = threadIdx.x;
  Elem* E = &D.el[e];
  if (!E->live) return;
  const int n_cand = E->n_cand, n_clu = E->n_cluster;
  if (n_cand == 0) return;
  for (int w = lane; w < D.kwords; w += 64) acc[w] = 0ull;
  __syncthreads();
  int count = 0, overflow = 0;
  const int* cd = D.cand + (size_t)e * D.kcap;
  const uint8_t* cc = D.can_clu + (size_t)e * D.kcap;
  int* cl = D.cluster + (size_t)e * D.ccap;
  int* ac = D.active + (size_t)e * D.ccap;
  uint8_t* fl = D.flags + (size_t)e * D.G;
  constexpr int kW = 4;  // row words per lane held in registers: candidates up to 64 * 64 * kW
  auto load_row = [&](int i, unsigned long long* r, int& okc, int& pc) {
    okc = cc[i] != 0;
    pc = cd[i];
    const unsigned long long* row = D.blocked + ((size_t)e * D.kcap + i) * D.kwords;
    const int nw = (i + 63) / 64;
#pragma unroll
    for (int q = 0; q < kW; q++) {
      const int w = lane + 64 * q;
      r[q] = (okc && w < nw) ? row[w] : 0ull;  // rows of rejected candidates were never written
    }
  };
  unsigned long long rn[kW];
  int okn, pn;
  load_row(0, rn, okn, pn);
  for (int i = 0; i < n_cand; i++) {
    unsigned long long r[kW];
#pragma unroll
    for (int q = 0; q < kW; q++) r[q] = rn[q];
    int ok = okn;
    const int p = pn;
    if (i + 1 < n_cand) load_row(i + 1, rn, okn, pn);
    if (ok) {
      int hit = 0;
#pragma unroll
      for (int q = 0; q < kW; q++) {
        const int w = lane + 64 * q;
        if (w < D.kwords) hit |= (r[q] & acc[w]) != 0ull;
      }
      for (int w = lane + 64 * kW; w < (i + 63) / 64; w += 64)  // beyond the registers (more than 16384 candidates)
        hit |= (D.blocked[((size_t)e * D.kcap + i) * D.kwords + w] & acc[w]) != 0ull;
      ok = !__any(hit);
    }
    if (lane == 0) {
      D.accept[(size_t)e * D.kcap + i] = (uint8_t)ok;
      if (ok) {
        acc[i >> 6] |= 1ull << (i & 63);
        if (n_clu + count < D.ccap) { cl[n_clu + count] = p; ac[count] = p; }
        else overflow = 1;
      } else {
        fl[px(p) * D.max_yz + py(p) * D.max_z + pz(p)] |= F_INVALID;  // CS:380-383
      }
    }
    count += ok;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  overflow = __any(overflow);
  if (lane == 0) {
    if (overflow) { E->rtn = DIRECT_CLUSTER_OVERFLOW; E->live = 0; E->n_cluster = D.ccap; E->n_active = 0; }
    else {
      E->n_cluster = n_clu + count;
      E->n_active = count;
      if (count == 0) E->live = 0;  // CS:386-387
      else E->iters += 1;           // CS:389
    }
  }
}

// candidates [i0, i1) of the accept loop with KW row words per lane (see k_resolve_fast)
template <int KW>
__device__ __forceinline__ void resolve_range(const Dev& D, int e, int lane, const unsigned long long* ccm, unsigned long long* acc, int i0, int i1) {
  constexpr int KG = 32 / KW;
  unsigned long long bufA[KG][KW], bufB[KG][KW];
  int okA[KG], okB[KG];
  auto load_group = [&](int g0, unsigned long long (*buf)[KW], int* okv) {
    // a group lies inside one 64-candidate word of the cluster-test mask (KG divides 64, i0 is a multiple of 4096)
    const int gw = (g0 < i1 ? g0 : i0) >> 6;
    unsigned long long gm = 0ull;
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (q == (gw >> 6)) gm = __shfl(ccm[q], gw & 63);
#pragma unroll
    for (int j = 0; j < KG; j++) {
      const int i = g0 + j;
      const int ic = i < i1 ? i : i0;
      const int okc = i < i1 ? (int)((gm >> (i & 63)) & 1ull) : 0;
      okv[j] = okc;
      const unsigned long long* row = D.blocked + ((size_t)e * D.kcap + ic) * D.kwords;
      const int nw = (i + 63) / 64;
#pragma unroll
      for (int q = 0; q < KW; q++) {
        const int w = lane + 64 * q;
        buf[j][q] = (okc && w < nw) ? row[w] : 0ull;  // rows of rejected candidates were never written
      }
    }
  };
  auto eval_group = [&](int g0, unsigned long long (*buf)[KW], const int* okv) {
#pragma unroll
    for (int j = 0; j < KG; j++) {
      const int i = g0 + j;
      if (i >= i1 || !okv[j]) continue;  // uniform
      int hit = 0;
#pragma unroll
      for (int q = 0; q < KW; q++) hit |= (buf[j][q] & acc[q]) != 0ull;
      if (__any(hit)) continue;
      const int w = i >> 6;
#pragma unroll
      for (int q = 0; q < 4; q++)
        if (q == (w >> 6) && lane == (w & 63)) acc[q] |= 1ull << (i & 63);
    }
  };
  load_group(i0, bufA, okA);
  for (int g0 = i0; g0 < i1; g0 += 2 * KG) {
    load_group(g0 + KG, bufB, okB);
    eval_group(g0, bufA, okA);
    load_group(g0 + 2 * KG, bufA, okA);
    eval_group(g0 + KG, bufB, okB);
  }
}

// The accept loop without a memory round trip on its serial chain (candidate capacities up to 64 * 64 * 4 = 16384; k_resolve_pipe
// above stays for larger ones).  The accepted-candidate bitset lives in REGISTERS (word w in lane w % 64, slot w / 64),
// the rows of the bit matrix arrive in groups of up to 32 candidates, two groups in flight, and nothing is written inside the
// loop: k_resolve_pipe's per-candidate stores needed a release fence, i.e. a wait for every outstanding load - the
// prefetched row included -, which made every candidate cost one global-memory latency (~1 us).  The decisions are the
// same sequence (candidate i joins iff it sees the old cluster and every earlier candidate that has joined); cluster /
// active appends, accept bytes and invalid flags are written afterwards by k_apply, one thread per candidate, from the bitset.
__global__ __launch_bounds__(64) void k_resolve_fast(Dev D) {
  const int e = blockIdx.x, lane = threadIdx.x;
  Elem* E = &D.el[e];
  if (!E->live) return;
  const int n_cand = E->n_cand, n_clu = E->n_cluster;
  if (n_cand == 0) return;
  const int* cd = D.cand + (size_t)e * D.kcap;
  const uint8_t* cc = D.can_clu + (size_t)e * D.kcap;
  constexpr int kW = 4;
  unsigned long long acc[kW] = {0ull, 0ull, 0ull, 0ull};
  // the cluster-test results as a bitset: word w (candidates 64 w ..) in lane w % 64, slot w / 64
  unsigned long long ccm[kW] = {0ull, 0ull, 0ull, 0ull};
  const int nwords = (n_cand + 63) / 64;
  for (int w0 = 0; w0 < nwords; w0 += 8) {
    int v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = (w0 + u) * 64 + lane;
      v[u] = (w0 + u < nwords && i < n_cand) ? (int)cc[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      // 1: joins unless an earlier accepted candidate is hidden from it (the sequential chain below); 2: sees everything
      // before it (k_convex): accepted at once - its bit can stand in acc from the start, rows only hold EARLIER candidates
      const unsigned long long m = __ballot(v[u] == 1), m2 = __ballot(v[u] == 2);
      const int w = w0 + u;
#pragma unroll
      for (int q = 0; q < kW; q++)
        if (q == (w >> 6) && lane == (w & 63)) { ccm[q] = m; acc[q] = m2; }
    }
  }
  // candidates below 4096 only meet row words below 64 (one per lane), below 8192 two per lane, ...: the narrower the
  // rows, the more candidates fit into the two groups in flight (32 / 16 / 8 per group)
  resolve_range<1>(D, e, lane, ccm, acc, 0, n_cand < 4096 ? n_cand : 4096);
  if (n_cand > 4096) resolve_range<2>(D, e, lane, ccm, acc, 4096, n_cand < 8192 ? n_cand : 8192);
  if (n_cand > 8192) resolve_range<4>(D, e, lane, ccm, acc, 8192, n_cand);
  // the bitset and its running counts for k_apply
  int count = 0;
#pragma unroll
  for (int q = 0; q < kW; q++) {
    const int c = __popcll(acc[q]);
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    const int w = q * 64 + lane;
    if (w < D.kwords) {
      D.accbits[(size_t)e * D.kwords + w] = acc[q];
      D.accpre[(size_t)e * D.kwords + w] = count + inc - c;
    }
    count += __shfl(inc, 63);
  }
  if (lane == 0) {
    E->pad0 = n_clu;  // where this round's voxels go (k_apply)
    // overflow: k_apply skips a dead element, so only the n_clu voxels of the earlier rounds are in the cluster array -
    // that valid prefix is what stays (slots beyond it were never written)
    if (n_clu + count > D.ccap) { E->rtn = DIRECT_CLUSTER_OVERFLOW; E->live = 0; E->n_cluster = n_clu; E->n_active = 0; }
    else {
      E->n_cluster = n_clu + count;
      E->n_active = count;
      if (count == 0) E->live = 0;  // CS:386-387
      else E->iters += 1;           // CS:389
    }
  }
}

// what the accept loop decided, applied in parallel: accepted candidates join the cluster and become the active set of
// the next round in candidate order (CS:371-379), the others are marked invalid (CS:380-383)
__global__ __launch_bounds__(256) void k_apply(Dev D) {
  const int e = blockIdx.y;
  const Elem* E = &D.el[e];
  if (!E->live) return;  // finished before this round, finished in it (nothing accepted), or overflowed (result not usable)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E->n_cand) return;
  const int w = i >> 6, b = i & 63;
  const unsigned long long word = D.accbits[(size_t)e * D.kwords + w];
  const int ok = (int)((word >> b) & 1ull);
  const int p = D.cand[(size_t)e * D.kcap + i];
  D.accept[(size_t)e * D.kcap + i] = (uint8_t)ok;
  if (ok) {
    const int r = D.accpre[(size_t)e * D.kwords + w] + __popcll(word & ((1ull << b) - 1ull));
    D.cluster[(size_t)e * D.ccap + E->pad0 + r] = p;
    D.active[(size_t)e * D.ccap + r] = p;
  } else {
    D.flags[(size_t)e * D.G + px(p) * D.max_yz + py(p) * D.max_z + pz(p)] |= F_INVALID;
  }
}

__global__ void k_emit(Dev D, int batch, int32_t* vertex_idx, int32_t* cluster_xyz, int32_t* cluster_num, int32_t* iters,
                       int32_t* rtn) {
  const int e = blockIdx.y;
  const Elem* E = &D.el[e];
  const int n = E->rtn == DIRECT_CLUSTER_BAD_SEED ? 0 : E->n_cluster;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {
    if (cluster_num) cluster_num[e] = n;
    if (iters) iters[e] = E->iters;
    if (rtn) rtn[e] = E->rtn;
  }
  if (vertex_idx && t < 24) vertex_idx[e * 24 + t] = E->vertex[t];
  if (cluster_xyz)
    for (int q = t; q < n; q += gridDim.x * blockDim.x) {
      const int p = D.cluster[(size_t)e * D.ccap + q];
      int32_t* o = cluster_xyz + ((size_t)e * D.ccap + q) * 3;
      o[0] = px(p); o[1] = py(p); o[2] = pz(p);
    }
  (void)batch;
}

#include "hull_kernels.h"
#include "grid_path.h"
#include "grid_path_clear.h"
#include "grid_path_fan.h"
#include "map_cloud.h"
#include "plan_check.h"
#include "dist_field.h"
#include "plan_clear.h"
#include "cube_corridor.h"
#include "cube_corridor_clear.h"
#include "free_comp.h"
#include "cluster_corridor.h"
#include "map_scan.h"
#include "map_evidence.h"
#include "map_close.h"
#include "frontier.h"
#include "view_gain.h"

thread_local std::string g_cerr;
direct_status_t cfail(direct_status_t st, const std::string& msg) {
  g_cerr = msg;
  return st;
}
#define CHIP_TRY(expr)                                                                             \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return cfail(DIRECT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));          \
  } while (0)

}  // namespace

struct direct_cluster_handle_s {
  direct_cluster_config_t cfg = {};
  Dev D = {};
  uint8_t* map = nullptr;
  uint8_t* inside_tmp = nullptr;
  int* seeds = nullptr;
  int32_t *st_vertex = nullptr, *st_xyz = nullptr, *st_num = nullptr, *st_iters = nullptr, *st_rtn = nullptr;  // device staging of host outputs
  hipStream_t stream = nullptr;
  hs::EventPair ev;  // direct_cluster_last_ms
  std::vector<void*> allocs;
  HullDev H = {};          // scratch of hull_planes_batch, allocated by its first call
  bool have_hull = false;
  int convex_grid = 2048;    // workgroups per seed of k_convex (DIRECT_CLUSTER_CONVEX_GRID: experiments)
  rs::State rs = {};         // what of all this is resident and still describes the map: the one owner (resident_state.h)
  hs::Block hull_out;        // device staging of its host outputs
  PathDev P = {};            // workspace of grid_path_batch, allocated by its first call (never shrunk, freed in destroy)
  bool have_path = false;
  hs::Block path_out;        // the read-back ring and the device staging of its host outputs, grown with path_capacity
  hs::Block cloud_in;        // device staging of a host cloud of map_from_cloud, grown on demand
  unsigned long long* cloud_cnt = nullptr;  // [2] its counters
  hs::Block plan_ws;  // workspace of plan_check_batch (counters, start times, per-slot leaves, unresolved list), grown on demand
  hs::Block plan_io;  // device staging of its host arrays, grown on demand
  int32_t* dist[2] = {nullptr, nullptr};  // the distance field (in dist[0]) and its ping-pong partner, allocated by the first distance_field
  unsigned long long* dist_cnt = nullptr;  // [2] the counters behind its stats
  double* path_pen = nullptr;  // [gp::kMaxPenalty] the penalty table of grid_path_clear_batch, allocated by its first call with a table
  hs::Block clear_ws;  // workspace of plan_clearance_batch (start times, per-slot minima), grown on demand
  hs::Block clear_io;  // device staging of its host arrays, grown on demand
  hs::Block cube_ws;   // workspace of cube_corridor_batch (the cube of every path slot, the walks' stacks), grown on demand
  hs::Block cube_in, cube_out;  // device staging of its host inputs / host outputs (two memory kinds: two blocks), grown on demand
  hs::Block fan_ws;    // workspace of grid_path_fan_batch (goals, their grouping, bounds, one read-back ring or two per goal), grown on demand
  hs::Block fan_out;   // device staging of its host outputs, grown on demand
  int fan_bound_every = 1;  // rounds between two k_fan_bound launches: 1 or 8 (DIRECT_CLUSTER_FAN_BOUND_EVERY: experiments)
  int* floor_tab[cc::kFloorSlots] = {};        // floor tables of cube_corridor_clear_batch (layout of D.sat), allocated by its first clear-mode call
  int32_t *comp_label = nullptr, *comp_size = nullptr;  // labels and sizes of free_components, allocated by its first call
  unsigned long long* comp_cnt = nullptr;  // [4] the counters behind its stats and its error word
  hs::Block reach_in, reach_out;  // device staging of reachable_batch's host inputs / host outputs, grown on demand
  hs::Block corr_ws;   // workspace of corridor_batch (walk states, plane stacks, owner table, seed list, a chunk's hull outputs), grown on demand
  hs::Block corr_in, corr_out;  // device staging of its host inputs / host outputs, grown on demand
  uint8_t* scan_raw = nullptr;            // the scan grid of map_integrate_scan (the map's size and layout), allocated by its first call
  unsigned long long* scan_cnt = nullptr; // [kScanCounters] its counters
  hs::Block scan_ws;                      // the two intermediate grids of its inflation, grown by the first call that inflates in y or z
  bool scan_test_store = true;            // the carve loads a byte before it stores (DIRECT_CLUSTER_SCAN_STORE=plain: experiments)
  bool scan_timing = false;               // record the phases' events (DIRECT_CLUSTER_SCAN_TIMING=1: tools/map_scan_bench.py)
  hipEvent_t scan_ev[5] = {};             // before the carve, behind the carve, the mark, the inflation and the table
  float scan_ms[4] = {0, 0, 0, 0};        // what they measured in the last call (the table: 0 when it was not rebuilt)
  uint8_t* known = nullptr;               // the known grid (the map's size and layout), allocated by the first tracked scan or set_known
  hs::Block known_in;                     // device staging of set_known's host bytes
  hs::Block front_ws;                     // workspace of frontier (mask, labels, sizes, slot grid, workgroup counts, counters), grown on demand
  hs::Block front_out;                    // its slot arrays and the device staging of its host outputs, grown with capacity
  hipEvent_t front_ev[5] = {};            // scan_timing: before the mask, behind the mask, the labelling, the compaction and the goals
  float front_ms[4] = {0, 0, 0, 0};
  bool front_timed = false;
  hs::Block view_in, view_out;            // device staging of view_gain_batch's host inputs / its error word and host outputs, grown on demand
  int view_threads = 0;                   // threads per workgroup of k_view_gain, 0: kViewThreads (DIRECT_CLUSTER_VIEW_THREADS: experiments)
  int8_t* evid = nullptr;                 // the evidence grid (the map's size and layout), allocated by the first evidence scan or set_evidence
  unsigned long long* evid_cnt = nullptr; // [kEvidCounters] the fold's counters
  hipEvent_t evid_ev[6] = {};             // scan_timing: before the touch, behind the touch, the hit, the fold, the inflation and the table
  float evid_ms[5] = {0, 0, 0, 0, 0};
  bool evid_timed = false;
  int32_t unknown_policy = DIRECT_UNKNOWN_FREE;  // what the NEXT scan does with unobserved voxels (direct_cluster_set_unknown_policy)
  uint8_t* open_map = nullptr;             // the open map (the map's size and layout), allocated by the first scan under DIRECT_UNKNOWN_OCCUPIED
  unsigned long long* close_cnt = nullptr; // [kCloseCounters] the close pass's own counters
  int64_t close_stats[2] = {0, 0};         // closed, open_ones of the last successful scan under the policy
};

namespace {
// The obstacles' summed-area table for k_convex's box test, from the map resident in h->map: the ONE place that builds it
// (direct_cluster_set_map and direct_cluster_map_from_cloud both end here).  Enqueues only.
hipError_t rebuild_sat(direct_cluster_handle_t h) {
  const Dev& D = h->D;
  hipLaunchKernelGGL(k_sat_fill, dim3(1024), dim3(256), 0, h->stream, D);
  for (int axis = 2; axis >= 0; axis--) hipLaunchKernelGGL(k_sat_scan, dim3(256), dim3(256), 0, h->stream, D, axis);
  return hipGetLastError();
}

// The workspace the two grid-path calls share (fields, flags, counters), allocated by whichever comes first: all or nothing, as
// the hull's scratch.
hipError_t path_workspace(direct_cluster_handle_t h) {
  if (h->have_path) return hipSuccess;
  const Dev& D = h->D;
  const size_t B = h->cfg.max_batch;
  PathDev N = {};
  N.X = D.max_x; N.Y = D.max_y; N.Z = D.max_z; N.YZ = D.max_yz; N.G = D.G;
  N.tx = gp::tiles_along(N.X); N.ty = gp::tiles_along(N.Y); N.tz = gp::tiles_along(N.Z);
  N.ntiles = N.tx * N.ty * N.tz;
  N.map = h->map;
  const hipError_t ae = hs::alloc_all(h->allocs, {
      hs::want(&N.field, B * (size_t)N.G * sizeof(double)), hs::want(&N.flag[0], B * (size_t)N.ntiles),
      hs::want(&N.flag[1], B * (size_t)N.ntiles), hs::want(&N.ends, B * 6 * sizeof(int)), hs::want(&N.pending, B * sizeof(int)),
      hs::want(&N.rounds, B * sizeof(int)), hs::want(&N.visits, B * sizeof(int))});
  if (ae != hipSuccess) return ae;
  h->P = N;
  h->have_path = true;
  return hipSuccess;
}

// The rounds of the three grid-path calls.  Rounds are separate launches, enqueued blindly gp::kFanRoundsPerCheck at a time (a
// workgroup whose tile is not active returns at once); then ONE read-back of the first n_slots "a tile was woken in round r"
// words says whether any slot goes on.  enqueue(r) launches round r.  *rounds_done counts the rounds enqueued, also on an error.
template <class Enqueue>
hipError_t path_rounds(direct_cluster_handle_t h, size_t n_slots, long long lim, int* rounds_done, Enqueue enqueue) {
  std::vector<int> pending(n_slots);
  int done = 0;
  while (done < lim) {
    const int n = (int)std::min<long long>(gp::kFanRoundsPerCheck, lim - done);
    for (int r = 0; r < n; r++) enqueue(done + r);
    hipError_t e = hipGetLastError();
    done += n;
    *rounds_done = done;
    if (e == hipSuccess) e = hipMemcpyAsync(pending.data(), h->P.pending, n_slots * sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return e;
    bool live = false;
    for (int v : pending) live |= v == done;
    if (!live) break;
  }
  return hipSuccess;
}

// The clearance parameters of grid_path_clear_batch and grid_path_fan_batch, in two steps, because what the arguments alone
// decide is refused before what the handle holds: each gives the refusal's text, or null.  This is the first; the second is
// rs::State::field_refusal.
const char* clear_args_refusal(int32_t min_d2, int32_t n_penalty, const double* penalty) {
  if (min_d2 < 0) return "min_d2 must not be negative";
  if (n_penalty < 0 || n_penalty > gp::kMaxPenalty) return "n_penalty outside [0, 65536]";
  if (n_penalty > 0 && !penalty) return "a NULL penalty requires n_penalty == 0";
  for (int i = 0; i < n_penalty; i++)
    if (!std::isfinite(penalty[i]) || !(penalty[i] >= 0.0)) return "penalty entries must be finite and not negative";
  return nullptr;
}

// a memory kind of the C-ABI, and what every call says to anything else
const char* const kMemRefusal = "mem is neither DIRECT_MEM_HOST nor DIRECT_MEM_DEVICE";
bool mem_kind(int32_t mem) { return mem == DIRECT_MEM_HOST || mem == DIRECT_MEM_DEVICE; }

// The penalty table on the device: path_pen, allocated by the first call with a table, and the upload of this call's entries
direct_status_t upload_penalty(direct_cluster_handle_t h, int32_t n_penalty, const double* penalty, const char* who) {
  if (n_penalty <= 0) return DIRECT_OK;
  if (!h->path_pen) {
    const hipError_t ae = hs::alloc_all(h->allocs, {hs::want(&h->path_pen, (size_t)gp::kMaxPenalty * sizeof(double))});
    if (ae != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string(who) + ": table allocation: " + hipGetErrorString(ae));
  }
  CHIP_TRY(hipMemcpyAsync(h->path_pen, penalty, (size_t)n_penalty * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return DIRECT_OK;
}

// plan_check_batch and plan_clearance_batch, whose input structs share their field names.  What both refuse comes in two ordered
// groups, each call having checks of its own between and behind them; `extent` is the call's one length, margin or radius.
template <class In, class Out>
const char* plan_rows_refusal(direct_cluster_handle_t h, const In* in, const Out* out) {
  if (!h || !in || !out || !in->n_seg || !in->T || !out->status) return "null argument";
  if (in->batch <= 0 || in->n_seg_max <= 0) return "batch and n_seg_max must be positive";
  if ((in->bez != nullptr) == (in->poly != nullptr)) return "exactly one of bez and poly";
  if (!mem_kind(in->mem)) return kMemRefusal;
  if (in->dtype != DIRECT_F32 && in->dtype != DIRECT_F64) return "dtype is neither DIRECT_F32 nor DIRECT_F64";
  if (in->depth < 0 || in->depth > pk::kMaxDepth) return "depth outside [0, 12]";
  return nullptr;
}
template <class In>
const char* plan_map_refusal(direct_cluster_handle_t h, const In* in, double extent, const char* extent_refusal) {
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) return "resolution must be finite and positive";
  if (!std::isfinite(extent) || !(extent >= 0.0)) return extent_refusal;
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(in->map_lower[a])) return "map_lower must be finite";
  return h->rs.has_map() ? nullptr : "the handle has no map";
}
// Their last refusal, then the row view (without S), the grid fields both Grids have and the four inputs on the call's Stage
template <class In, class Grid>
direct_status_t plan_rows_stage(direct_cluster_handle_t h, hs::Stage& st, const In* in, PlanRows& R, Grid& G) {
  const size_t B = (size_t)in->batch, slots = B * (size_t)in->n_seg_max, r = in->dtype == DIRECT_F32 ? sizeof(float) : sizeof(double);
  if (slots >= (1ull << 31)) return cfail(DIRECT_ERR_UNSUPPORTED, "batch * n_seg_max of 2^31 or more");
  CHIP_TRY(hipSetDevice(h->cfg.device));
  for (int a = 0; a < 3; a++) G.lower[a] = in->map_lower[a];
  G.inv = 1.0 / in->resolution;
  G.size[0] = h->D.max_x; G.size[1] = h->D.max_y; G.size[2] = h->D.max_z;
  R.batch = in->batch; R.nmax = in->n_seg_max; R.depth = in->depth; R.poly = in->poly != nullptr; R.has_from = in->t_from != nullptr;
  hs::stage_in(st, &R.n_seg, in->n_seg, B * 4);
  hs::stage_in(st, &R.T, in->T, slots * r);
  hs::stage_in(st, &R.coef, in->poly ? in->poly : in->bez, slots * 18 * r);
  hs::stage_in(st, &R.t_from, in->t_from, B * 8);
  return DIRECT_OK;
}
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }  // bytes rounded up to the 256-byte pieces both workspaces are laid out in
// Their timed part and way back, after stage_upload: launch() enqueues the kernels between the handle's two events, the staged
// outputs come back, after() enqueues what else the call reads, the stream drains.  `who` opens the message of a device error.
template <class Launch, class After>
direct_status_t plan_run(direct_cluster_handle_t h, const hs::Stage& st, const char* who, Launch launch, After after) {
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = launch();
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  e = hs::stage_download(st, h->stream, e);
  if (e == hipSuccess) e = after();
  e = hs::drain(h->stream, e);
  return e == hipSuccess ? DIRECT_OK : cfail(DIRECT_ERR_DEVICE, std::string(who) + hipGetErrorString(e));
}

// what the fetch and reachable_batch say to a label set that is missing or older than the map (or, built with a floor, the field)
const char* const kCompStale = "no valid free components: call direct_cluster_free_components after the map or the distance field changes";

PathClearDev clear_dev(direct_cluster_handle_t h, int32_t min_d2, int32_t n_penalty) {
  PathClearDev C = {};
  C.d2 = h->dist[0];
  C.pen = n_penalty > 0 ? h->path_pen : nullptr;
  C.n_pen = n_penalty; C.min_d2 = min_d2;
  return C;
}

// PathDev::ends of n slots on the host (the caller keeps it alive until its copy has drained)
std::vector<int> pack_ends(size_t n, const int32_t* starts, const int32_t* goals) {
  std::vector<int> ends(n * 6);
  for (size_t b = 0; b < n; b++)
    for (int a = 0; a < 3; a++) { ends[6 * b + a] = starts[3 * b + a]; ends[6 * b + 3 + a] = goals[3 * b + a]; }
  return ends;
}

// the fields of n slots to the caller's `dist` (null: nothing), unless e already holds an error
hipError_t download_fields(direct_cluster_handle_t h, double* dist, size_t n, int32_t mem, hipError_t e) {
  if (e != hipSuccess || !dist) return e;
  return hipMemcpyAsync(dist, h->P.field, n * (size_t)h->P.G * sizeof(double),
                        mem == DIRECT_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream);
}

// grid_path_batch, grid_path_clear_batch and grid_path_fan_batch behind their refusals: what one call is ...
struct PathCall {
  const char* who;                 // opens its messages
  int n_field, n_path;             // fields relaxed (at most max_batch), paths read back from them
  int32_t path_capacity, max_rounds, mem;
  const int32_t *starts, *goals;   // [n_field][3] each: every field's (start, goal); the fan passes its sources for both
  bool clear;                      // reads the distance field under (min_d2, the n_penalty entries of penalty)
  int32_t min_d2, n_penalty;
  const double* penalty;
  double* dist;                    // the caller's array for the fields, or null
};
// ... and what all three do.  stage(P, C) registers what is left to register and uploads the call's blocks (its refusal ends the
// call), relax(P, C, r) launches round r, trace(P, C, done) the read-back; `out` is the Stage whose outputs go back.
template <class StageFn, class Relax, class Trace>
direct_status_t grid_path_run(direct_cluster_handle_t h, const PathCall& c, const hs::Stage& out, StageFn stage, Relax relax, Trace trace) {
  const std::string who(c.who);
  if (const hipError_t ae = path_workspace(h); ae != hipSuccess)
    return cfail(DIRECT_ERR_DEVICE, who + ": workspace allocation: " + hipGetErrorString(ae));
  if (const direct_status_t us = upload_penalty(h, c.n_penalty, c.penalty, c.who); us != DIRECT_OK) return us;
  PathDev& P = h->P;
  PathClearDev C = c.clear ? clear_dev(h, c.min_d2, c.n_penalty) : PathClearDev{};
  if (const direct_status_t rc = stage(P, C)) return rc;
  P.cap = c.path_capacity;
  const size_t nf = (size_t)c.n_field;
  const std::vector<int> ends = pack_ends(nf, c.starts, c.goals);
  CHIP_TRY(hipMemcpyAsync(P.ends, ends.data(), nf * 6 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipLaunchKernelGGL(k_path_init, dim3(std::min((P.G + 255) / 256, 2048), c.n_field), dim3(256), 0, h->stream, P);
  CHIP_TRY(hipGetLastError());
  const long long lim = c.max_rounds > 0 ? (long long)c.max_rounds : gp::default_max_rounds(P.X, P.Y, P.Z);
  int done = 0;
  hipError_t e = path_rounds(h, nf, lim, &done, [&](int r) { relax(P, C, r); });
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, who + ": rounds: " + hipGetErrorString(hs::drain(h->stream, e)));
  trace(P, C, done);
  e = hipGetLastError();
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  e = hs::drain(h->stream, download_fields(h, c.dist, nf, c.mem, hs::stage_download(out, h->stream, e)));
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, who + ": " + hipGetErrorString(e));
  return DIRECT_OK;
}
// The stage() of grid_path_batch and grid_path_clear_batch, one path per field: ONE block, path_out, for the read-back rings (scratch
// slices, needed whatever `mem` is; the ring of D2 values in clear mode only) and the staging of host outputs (nothing is filled).
// user / dev: path_xyz, path_len, path_cost, stats, rtn, path_d2, path_min_d2 - the last two null outside clear mode.
direct_status_t path_pair_stage(direct_cluster_handle_t h, const PathCall& c, hs::Stage& st, PathDev& P, PathClearDev& C, void* const* user, void** dev) {
  const size_t nb = (size_t)c.n_path, cap = (size_t)c.path_capacity;
  const size_t sz[7] = {nb * cap * 3 * sizeof(int32_t), nb * sizeof(int32_t), nb * sizeof(double), nb * 2 * sizeof(int32_t), nb * sizeof(int32_t),
                        nb * cap * sizeof(int32_t), nb * sizeof(int32_t)};
  hs::stage_scratch(st, &P.ring, nb * cap * sizeof(int));
  if (c.clear) hs::stage_scratch(st, &C.ring_d2, nb * cap * sizeof(int));
  for (int i = 0; i < 7; i++) hs::stage_out(st, &dev[i], user[i], sz[i]);
  CHIP_TRY(hs::stage_upload(st, h->path_out, h->stream));
  return DIRECT_OK;
}

// map_from_cloud and map_integrate_scan: what both refuse of a cloud - the points and their memory kind first in both, the stride
// and the resolution where each call has them among its own checks ...
const char* cloud_refusal(int64_t n_points, int32_t mem, const float* xyz) {
  if (n_points < 0 || (n_points > 0 && !xyz)) return "n_points negative, or points without a pointer";
  return mem_kind(mem) ? nullptr : kMemRefusal;
}
const char* stride_refusal(int32_t stride) { return stride != 3 && stride != 4 ? "stride must be 3 or 4 floats per point" : nullptr; }
const char* resolution_refusal(double resolution) {
  return !std::isfinite(resolution) || !(resolution > 0.0) ? "resolution must be finite and positive" : nullptr;
}
// ... and the cloud on the device: the caller's own pointer, or a host cloud's copy in cloud_in (enqueued)
direct_status_t cloud_on_device(direct_cluster_handle_t h, int64_t n_points, int32_t stride, int32_t mem, const float* xyz, const float** dev) {
  *dev = xyz;
  if (mem != DIRECT_MEM_HOST || n_points <= 0) return DIRECT_OK;
  const size_t bytes = (size_t)n_points * stride * sizeof(float);
  CHIP_TRY(hs::grow(h->cloud_in, h->stream, bytes));
  CHIP_TRY(hipMemcpyAsync(h->cloud_in.p, xyz, bytes, hipMemcpyHostToDevice, h->stream));
  *dev = (const float*)h->cloud_in.p;
  return DIRECT_OK;
}

// The four fetches behind their refusals: one resident array, or two of one size, to the caller in either memory kind (a null
// destination is skipped), and the drain
direct_status_t fetch_resident(direct_cluster_handle_t h, int32_t mem, size_t bytes, void* dst, const void* src, void* dst2 = nullptr,
                               const void* src2 = nullptr) {
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const hipMemcpyKind kind = mem == DIRECT_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (dst) CHIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, h->stream));
  if (dst2) CHIP_TRY(hipMemcpyAsync(dst2, src2, bytes, kind, h->stream));
  CHIP_TRY(hipStreamSynchronize(h->stream));
  return DIRECT_OK;
}

// cube_corridor_batch, cube_corridor_clear_batch and corridor_batch, whose structs share these field names.  What all refuse, in
// the plain call's order; DIRECT_OK: nothing to refuse.
// `more` is a further refusal that the call's arguments alone decide (or null): it comes before what the handle holds.
template <class In, class Out>
direct_status_t cube_corridor_refusal(direct_cluster_handle_t h, const In* in, const Out* out, const char* more) {
  if (!h || !in || !out || !in->path_xyz || !in->path_len) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (in->batch <= 0 || in->path_capacity <= 0 || in->seg_capacity <= 0 || in->itr_inflate_max <= 0)
    return cfail(DIRECT_ERR_INVALID, "batch, path_capacity, seg_capacity and itr_inflate_max must be positive");
  if (in->p_max < cc::kPlanes) return cfail(DIRECT_ERR_INVALID, "p_max below 6");
  if (!mem_kind(in->mem_in) || !mem_kind(out->mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (in->plane_dtype != DIRECT_F32 && in->plane_dtype != DIRECT_F64) return cfail(DIRECT_ERR_INVALID, "plane_dtype is neither DIRECT_F32 nor DIRECT_F64");
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) return cfail(DIRECT_ERR_INVALID, "resolution must be finite and positive");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(in->map_lower[a])) return cfail(DIRECT_ERR_INVALID, "map_lower must be finite");
  if (more) return cfail(DIRECT_ERR_INVALID, more);
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  const size_t B = (size_t)in->batch, slots = B * (size_t)in->path_capacity, segs = B * (size_t)in->seg_capacity;
  if (slots >= (1ull << 28) || segs * (size_t)in->p_max >= (1ull << 28))
    return cfail(DIRECT_ERR_UNSUPPORTED, "batch * path_capacity or batch * seg_capacity * p_max of 2^28 or more");
  return DIRECT_OK;
}
// Their workspace, staging, launches and way back, after cube_corridor_refusal and hipSetDevice.  D is the handle's Dev, or a copy
// whose `sat` is a floor table: the slab test counts what that table counts.  before() enqueues what the table still needs, behind
// the first of the handle's two events; after() enqueues what else the call reads.  `who` opens the message of a device error.
template <class Before, class After>
direct_status_t cube_corridor_run(direct_cluster_handle_t h, const direct_cube_corridor_in_t* in, direct_cube_corridor_out_t* out, const Dev& D,
                                  const char* who, Before before, After after) {
  const size_t B = (size_t)in->batch, slots = B * (size_t)in->path_capacity, segs = B * (size_t)in->seg_capacity;
  const size_t w_stack = (slots * 6 * sizeof(int) + 255) & ~(size_t)255;
  CHIP_TRY(hs::grow(h->cube_ws, h->stream, w_stack + slots * sizeof(int)));
  CubeDev A = {};
  A.batch = in->batch; A.path_cap = in->path_capacity; A.seg_cap = in->seg_capacity; A.p_max = in->p_max;
  A.itr_inflate_max = in->itr_inflate_max; A.pop_back = in->pop_back ? 1 : 0;
  A.res = in->resolution;
  for (int a = 0; a < 3; a++) A.lower[a] = in->map_lower[a];
  A.cube = (int*)h->cube_ws.p;
  A.stack = (int*)((char*)h->cube_ws.p + w_stack);
  const size_t r = in->plane_dtype == DIRECT_F32 ? sizeof(float) : sizeof(double);
  hs::Stage si(in->mem_in == DIRECT_MEM_HOST), so(out->mem == DIRECT_MEM_HOST);
  hs::stage_in(si, &A.path_xyz, in->path_xyz, slots * 3 * sizeof(int32_t));
  hs::stage_in(si, &A.path_len, in->path_len, B * sizeof(int32_t));
  hs::stage_out(so, &A.n_seg, out->n_seg, B * sizeof(int32_t));
  hs::stage_out(so, &A.n_planes, out->n_planes, segs * sizeof(int32_t));
  hs::stage_out(so, &A.planes, out->planes, segs * (size_t)in->p_max * 4 * r);
  hs::stage_out(so, &A.seeds, out->seeds, segs * 3 * r);
  hs::stage_out(so, &A.centers, out->centers, segs * 3 * r);
  hs::stage_out(so, &A.cube_idx, out->cube_idx, segs * 6 * sizeof(int32_t));
  hs::stage_out(so, &A.rtn, out->rtn, B * sizeof(int32_t));
  CHIP_TRY(hs::stage_upload(si, h->cube_in, h->stream));
  CHIP_TRY(hs::stage_upload(so, h->cube_out, h->stream));
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = before();
  if (e == hipSuccess) {
    const int blocks = (int)std::min<size_t>((slots + 63) / 64, 8192);  // a fixed grid beyond 524288 slots: the lanes stride
    hipLaunchKernelGGL(k_cube_inflate, dim3(blocks), dim3(64), 0, h->stream, D, A);
    if (in->plane_dtype == DIRECT_F32) hipLaunchKernelGGL(k_cube_walk<float>, dim3(in->batch), dim3(64), 0, h->stream, A);
    else hipLaunchKernelGGL(k_cube_walk<double>, dim3(in->batch), dim3(64), 0, h->stream, A);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  e = hs::stage_download(so, h->stream, e);
  if (e == hipSuccess) e = after();
  e = hs::drain(h->stream, e);
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string(who) + hipGetErrorString(e));
  return DIRECT_OK;
}

// The device part of polygon_generation_batch for `batch` <= max_batch seeds in DEVICE memory (seeds[batch][3]): flagClear, the
// cube, the rounds of polytopeCluster_cpu and the emit into DEVICE outputs (any may be null).  Enqueues on the handle's stream and
// waits for its own liveness read-backs, the last of which leaves the elements' counters in `el`; events, the copies of host arrays
// and what the handle's rs hears of the clusters are the caller's.
direct_status_t generation_run(direct_cluster_handle_t h, int batch, const int* seeds, int itr_inflate_max, int itr_cluster_max, int32_t* dv,
                               int32_t* dc, int32_t* dn, int32_t* di, int32_t* dr, std::vector<Elem>& el) {
  Dev& D = h->D;
  const int gblocks = std::min((D.G + 255) / 256, 4096);
  hipLaunchKernelGGL(k_flags_init, dim3(gblocks, batch), dim3(256), 0, h->stream, D, (const uint8_t*)nullptr);  // flagClear CS:20-26
  hipLaunchKernelGGL(k_inflate, dim3(batch), dim3(256), 0, h->stream, D, seeds, itr_inflate_max);
  CHIP_TRY(hipGetLastError());
  el.resize(batch);
  auto fetch = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(el.data(), D.el, (size_t)batch * sizeof(Elem), hipMemcpyDeviceToHost, h->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
  };
  CHIP_TRY(fetch());
  // polytopeCluster_cpu (CS:295-392).  No launch of a round depends on a count the round produces (grid-stride or
  // capacity-sized kernels over device-resident counters; workgroups of finished seeds return at once), so the host enqueues rounds
  // blindly, kRoundsPerCheck at a time, and only then looks whether any seed is still growing: one read-back per
  // kRoundsPerCheck rounds instead of three per round (the reference's CUDA twin, cluster_server.cu:628-685, copies
  // per round as well).
  constexpr int kRoundsPerCheck = 4;
  for (int round = 0; round < itr_cluster_max;) {
    int live = 0;
    for (const Elem& E : el) live += E.live ? 1 : 0;
    if (!live) break;
    const int n = std::min(kRoundsPerCheck, itr_cluster_max - round);
    for (int r = 0; r < n; r++) {
      hipLaunchKernelGGL(k_mark, dim3(128, batch), dim3(256), 0, h->stream, D);
      hipLaunchKernelGGL(k_compact_count, dim3(kCompactBlocks, batch), dim3(256), 0, h->stream, D);
      hipLaunchKernelGGL(k_compact_write, dim3(kCompactBlocks, batch), dim3(256), 0, h->stream, D);
      // one workgroup per candidate SLOT: the slots beyond a seed's candidate count return at once (640 k empty
      // workgroups cost ~0.1 ms; a persistent ticket kernel with the rays' voxels staged in LDS was built and measured
      // 1.6 - 2 x slower: thousands of short workgroups balance the seeds' very different loads better, and the flag
      // bytes of a round's rays live in L2 anyway)
      hipLaunchKernelGGL(k_chunk_box, dim3(D.nchunk, batch), dim3(256), 0, h->stream, D);
      hipLaunchKernelGGL(k_convex<false>, dim3(std::min(D.kcap, h->convex_grid), batch), dim3(256), 0, h->stream, D);
      if (D.kwords <= 256) {
        hipLaunchKernelGGL(k_resolve_fast, dim3(batch), dim3(64), 0, h->stream, D);
        hipLaunchKernelGGL(k_apply, dim3((D.kcap + 255) / 256, batch), dim3(256), 0, h->stream, D);
      }
      else hipLaunchKernelGGL(k_resolve_pipe, dim3(batch), dim3(64), (size_t)D.kwords * 8, h->stream, D);
    }
    CHIP_TRY(hipGetLastError());
    round += n;
    CHIP_TRY(fetch());
  }
  hipLaunchKernelGGL(k_emit, dim3(64, batch), dim3(256), 0, h->stream, D, batch, dv, dc, dn, di, dr);
  return DIRECT_OK;
}

// The scratch of the hull kernels, allocated by the first call that needs it: all or nothing, so that a retry starts clean
direct_status_t hull_workspace(direct_cluster_handle_t h) {
  if (h->have_hull) return DIRECT_OK;
  const Dev& D = h->D;
  HullDev& H = h->H;
  const size_t B = h->cfg.max_batch;
  H.QX = 2 * D.max_x + 1; H.QY = 2 * D.max_y + 1; H.QZ = 2 * D.max_z + 1;
  H.half_words = (size_t)H.QY * H.QZ + (size_t)H.QX * H.QZ + (size_t)H.QX * H.QY;
  H.line_words = 2 * H.half_words;
  const hipError_t ae = hs::alloc_all(h->allocs, {
      hs::want(&H.he, B * sizeof(HullElem)), hs::want(&H.lines, B * H.line_words * sizeof(int)),
      hs::want(&H.cand, B * 3 * hull::kCandCap * sizeof(int)), hs::want(&H.first, B * hull::kCandCap * sizeof(int)),
      hs::want(&H.isv, B * hull::kCandCap * sizeof(int)), hs::want(&H.raw, B * hull::kRawCap * 4 * sizeof(hull::i64)),
      hs::want(&H.sorted, B * hull::kRawCap * 4 * sizeof(hull::i64)), hs::want(&H.vq, B * hull::kCandCap * 3 * sizeof(int))});
  if (ae != hipSuccess) {
    H = HullDev{};
    return cfail(DIRECT_ERR_DEVICE, std::string("hull_planes_batch: scratch allocation: ") + hipGetErrorString(ae));
  }
  h->have_hull = true;
  return DIRECT_OK;
}

// The device part of hull_planes_batch for `batch` <= max_batch clusters: sx / sn are DEVICE voxels and counts that replace the
// resident clusters, or null for the resident ones; dev[8] are DEVICE outputs in the public call's order (planes, plane_int,
// n_planes, vertices, n_vertices, center, degenerate, rtn), any may be null.  Enqueues only.
direct_status_t hull_run(direct_cluster_handle_t h, int batch, const int32_t* sx, const int32_t* sn, double resolution, const double* map_lower,
                         int plane_capacity, int vertex_capacity, void* const* dev) {
  Dev& D = h->D;
  HullDev& H = h->H;
  const size_t nb = (size_t)batch;
  CHIP_TRY(hipMemset2DAsync(H.lines, H.line_words * sizeof(int), 0x7f, H.half_words * sizeof(int), nb, h->stream));
  CHIP_TRY(hipMemset2DAsync(H.lines + H.half_words, H.line_words * sizeof(int), 0x80, H.half_words * sizeof(int), nb, h->stream));
  CHIP_TRY(hipMemsetAsync(H.he, 0, nb * sizeof(HullElem), h->stream));
  hipLaunchKernelGGL(k_hull_src, dim3(32, batch), dim3(256), 0, h->stream, D, H, batch, sx, sn);
  hipLaunchKernelGGL(k_hull_lines, dim3(batch), dim3(256), 0, h->stream, D, H);
  hipLaunchKernelGGL(k_hull_cand, dim3(batch), dim3(256), 0, h->stream, D, H);
  hipLaunchKernelGGL(k_hull_edges, dim3(64, batch), dim3(256), 0, h->stream, H);
  hipLaunchKernelGGL(k_hull_finish, dim3(batch), dim3(256), 0, h->stream, H, resolution, map_lower[0], map_lower[1], map_lower[2],
                     plane_capacity, vertex_capacity, (double*)dev[0], (long long*)dev[1], (int32_t*)dev[2], (double*)dev[3],
                     (int32_t*)dev[4], (double*)dev[5], (int32_t*)dev[6], (int32_t*)dev[7]);
  return DIRECT_OK;
}
}  // namespace

extern "C" {

const char* direct_cluster_last_error(void) { return g_cerr.c_str(); }

direct_status_t direct_cluster_create(const direct_cluster_config_t* cfg, direct_cluster_handle_t* out) {
  if (!cfg || !out) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (cfg->max_x <= 0 || cfg->max_y <= 0 || cfg->max_z <= 0 || cfg->max_batch <= 0 || cfg->cluster_capacity <= 0 ||
      cfg->candidate_capacity <= 0)
    return cfail(DIRECT_ERR_INVALID, "bad sizes");
  if (cfg->max_x > kDimLimit || cfg->max_y > kDimLimit || cfg->max_z > kDimLimit)
    return cfail(DIRECT_ERR_UNSUPPORTED, "map dimensions above 1024 voxels per axis");
  if ((long long)cfg->max_x * cfg->max_y * cfg->max_z > 0x7fffffffLL / 2) return cfail(DIRECT_ERR_UNSUPPORTED, "map too large");
  // the summed-area table has (X+1)(Y+1)(Z+1) int entries and box_obstacles addresses it with unsigned 32-bit BYTE offsets
  if ((long long)(cfg->max_x + 1) * (cfg->max_y + 1) * (cfg->max_z + 1) >= (1LL << 30))
    return cfail(DIRECT_ERR_UNSUPPORTED, "map too large: the summed-area table would exceed 4 GiB");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return cfail(DIRECT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return cfail(DIRECT_ERR_INVALID, "bad device ordinal");
  CHIP_TRY(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  CHIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return cfail(DIRECT_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  direct_cluster_handle_t h = new direct_cluster_handle_s();
  h->cfg = *cfg;
  if (const char* ev = getenv("DIRECT_CLUSTER_CONVEX_GRID")) h->convex_grid = atoi(ev) > 0 ? atoi(ev) : h->convex_grid;
  if (const char* ev = getenv("DIRECT_CLUSTER_SCAN_STORE")) h->scan_test_store = std::string(ev) != "plain";
  if (const char* ev = getenv("DIRECT_CLUSTER_SCAN_TIMING")) h->scan_timing = atoi(ev) > 0;
  if (const char* ev = getenv("DIRECT_CLUSTER_VIEW_THREADS")) h->view_threads = (atoi(ev) == 256 || atoi(ev) == 512 || atoi(ev) == 1024) ? atoi(ev) : 0;
  if (const char* ev = getenv("DIRECT_CLUSTER_FAN_BOUND_EVERY")) h->fan_bound_every = atoi(ev) == gp::kFanRoundsPerCheck ? gp::kFanRoundsPerCheck : 1;
  Dev& D = h->D;
  D.max_x = cfg->max_x; D.max_y = cfg->max_y; D.max_z = cfg->max_z; D.max_yz = cfg->max_y * cfg->max_z;
  D.G = cfg->max_x * cfg->max_y * cfg->max_z;
  D.ccap = cfg->cluster_capacity; D.kcap = cfg->candidate_capacity; D.kwords = (cfg->candidate_capacity + 63) / 64;
  const size_t B = cfg->max_batch, G = D.G;
  D.sat_z = cfg->max_z + 1; D.sat_yz = (cfg->max_y + 1) * D.sat_z;
  D.nchunk = (cfg->cluster_capacity + 255) / 256;
  float* invp = nullptr;
  const hipError_t ae = hs::alloc_all(h->allocs, {
      hs::want(&D.sat, (size_t)(cfg->max_x + 1) * D.sat_yz * sizeof(int)), hs::want(&invp, kDimLimit * sizeof(float)),
      hs::want(&D.cbox, B * (size_t)D.nchunk * 6 * sizeof(int)),
      hs::want(&h->map, G), hs::want(&h->inside_tmp, G), hs::want(&h->seeds, B * 3 * sizeof(int)),
      hs::want(&D.flags, B * G), hs::want(&D.key, B * G * sizeof(int)),
      hs::want(&D.cluster, B * D.ccap * sizeof(int)), hs::want(&D.active, B * D.ccap * sizeof(int)), hs::want(&D.cand, B * D.kcap * sizeof(int)),
      hs::want(&D.can_clu, B * D.kcap), hs::want(&D.accept, B * D.kcap),
      hs::want(&D.blocked, B * D.kcap * (size_t)D.kwords * sizeof(unsigned long long)),
      hs::want(&D.accbits, B * (size_t)D.kwords * sizeof(unsigned long long)), hs::want(&D.accpre, B * (size_t)D.kwords * sizeof(int)),
      hs::want(&D.el, B * sizeof(Elem)),
      hs::want(&D.ccnt, B * kCompactBlocks * sizeof(int)), hs::want(&D.csnap, B * 2 * sizeof(int)),
      hs::want(&h->st_vertex, B * 24 * 4), hs::want(&h->st_xyz, B * (size_t)D.ccap * 12), hs::want(&h->st_num, B * 4),
      hs::want(&h->st_iters, B * 4), hs::want(&h->st_rtn, B * 4)});
  direct_status_t st = ae == hipSuccess ? DIRECT_OK : cfail(DIRECT_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(ae));
  D.inv = invp;
  D.map = h->map;
  if (st == DIRECT_OK) {
    hipLaunchKernelGGL(k_inv_table, dim3(1), dim3(256), 0, nullptr, invp);
    if (hipDeviceSynchronize() != hipSuccess) st = cfail(DIRECT_ERR_DEVICE, "k_inv_table failed");
  }
  if (st == DIRECT_OK && hs::create(h->ev) != hipSuccess) st = cfail(DIRECT_ERR_DEVICE, "hipEventCreate failed");
  if (st != DIRECT_OK) {
    direct_cluster_destroy(h);
    return st;
  }
  *out = h;
  return DIRECT_OK;
}

direct_status_t direct_cluster_destroy(direct_cluster_handle_t h) {
  if (!h) return DIRECT_OK;
  (void)hipSetDevice(h->cfg.device);
  (void)hipDeviceSynchronize();
  for (void* p : h->allocs) (void)hipFree(p);
  for (hs::Block* b : {&h->hull_out, &h->path_out, &h->cloud_in, &h->plan_ws, &h->plan_io, &h->clear_ws, &h->clear_io, &h->cube_ws, &h->cube_in,
                       &h->cube_out, &h->fan_ws, &h->fan_out, &h->reach_in, &h->reach_out, &h->corr_ws, &h->corr_in, &h->corr_out, &h->scan_ws,
                       &h->known_in, &h->front_ws, &h->front_out, &h->view_in, &h->view_out})
    hs::release(*b);
  for (hipEvent_t e : h->scan_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->front_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->evid_ev)
    if (e) (void)hipEventDestroy(e);
  hs::destroy(h->ev);
  delete h;
  return DIRECT_OK;
}

direct_status_t direct_cluster_set_map(direct_cluster_handle_t h, int32_t mem, const uint8_t* map_data) {
  if (!h || !map_data) return cfail(DIRECT_ERR_INVALID, "null argument");
  h->rs.map_edit_began();  // the map is about to change: neither a distance field nor the labels of free_components describe it
  CHIP_TRY(hipSetDevice(h->cfg.device));
  CHIP_TRY(hipMemcpyAsync(h->map, map_data, (size_t)h->D.G, mem == DIRECT_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                          h->stream));
  CHIP_TRY(hipStreamSynchronize(h->stream));
  CHIP_TRY(rebuild_sat(h));
  CHIP_TRY(hipStreamSynchronize(h->stream));
  h->rs.map_ready();
  return DIRECT_OK;
}

direct_status_t direct_cluster_map_from_cloud(direct_cluster_handle_t h, const direct_map_cloud_t* p, int64_t n_points, int32_t mem,
                                              const float* xyz, int64_t* stats) {
  if (!h || !p) return cfail(DIRECT_ERR_INVALID, "null argument");
  h->rs.map_edit_began();  // whether or not the call succeeds: a distance field and the labels of free_components are rebuilt by its caller
  const char* why = cloud_refusal(n_points, mem, xyz);
  if (!why) why = resolution_refusal(p->resolution);
  if (!why && (!std::isfinite(p->cloud_margin) || !(p->cloud_margin >= 0.0))) why = "cloud_margin must be finite and not negative";
  if (!why) why = stride_refusal(p->stride);
  if (why) return cfail(DIRECT_ERR_INVALID, why);
  if (p->border != DIRECT_MAP_BORDER_CLAMP && p->border != DIRECT_MAP_BORDER_DROP) return cfail(DIRECT_ERR_INVALID, "unknown border convention");
  if (p->mode != DIRECT_MAP_REPLACE && p->mode != DIRECT_MAP_ADD) return cfail(DIRECT_ERR_INVALID, "unknown mode");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(p->map_lower[a]) || (p->border == DIRECT_MAP_BORDER_DROP && !std::isfinite(p->map_upper[a])))
      return cfail(DIRECT_ERR_INVALID, "map_lower / map_upper must be finite");
  const double inv = 1.0 / p->resolution;
  if (!(p->cloud_margin * inv < (double)mc::kMaxSteps + 0.5)) return cfail(DIRECT_ERR_UNSUPPORTED, "cloud_margin above 1024 voxel steps");
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const Dev& D = h->D;
  CloudDev C = {};
  for (int a = 0; a < 3; a++) { C.lower[a] = p->map_lower[a]; C.upper[a] = p->map_upper[a]; }
  C.resolution = p->resolution; C.inv = inv;
  C.size[0] = D.max_x; C.size[1] = D.max_y; C.size[2] = D.max_z;
  mc::inf_steps(p->cloud_margin, p->resolution, &C.s, &C.sz);
  C.border = p->border; C.stride = p->stride; C.n = n_points; C.map = h->map;
  if (!h->cloud_cnt) CHIP_TRY(hs::alloc_all(h->allocs, {hs::want(&h->cloud_cnt, 2 * sizeof(unsigned long long))}));
  C.cnt = h->cloud_cnt;
  if (const direct_status_t rc = cloud_on_device(h, n_points, p->stride, mem, xyz, &C.xyz)) return rc;
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = hipMemsetAsync(h->cloud_cnt, 0, 2 * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess && (p->mode == DIRECT_MAP_REPLACE || !h->rs.has_map())) e = hipMemsetAsync(h->map, 0, (size_t)D.G, h->stream);
  if (e == hipSuccess && n_points > 0) {
    const long long lanes = (long long)n_points * (2 * C.s + 1) * (2 * C.s + 1);
    const int blocks = (int)std::min<long long>((lanes + 255) / 256, 1 << 16);  // grid-stride beyond 16.8 M lanes
    hipLaunchKernelGGL(k_cloud_raster, dim3(blocks), dim3(256), 0, h->stream, C);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = rebuild_sat(h);
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  unsigned long long cnt[2] = {0, 0};
  int occupied = 0;  // the table's last entry is the sum over the whole map: the count and the table cannot disagree
  if (e == hipSuccess && stats) e = hipMemcpyAsync(cnt, h->cloud_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && stats)
    e = hipMemcpyAsync(&occupied, D.sat + ((size_t)(D.max_x + 1) * D.sat_yz - 1), sizeof(int), hipMemcpyDeviceToHost, h->stream);
  e = hs::drain(h->stream, e);
  // the map has been touched: whatever happened, an earlier table no longer describes it
  if (e != hipSuccess) {
    h->rs.map_lost();
    return cfail(DIRECT_ERR_DEVICE, std::string("map_from_cloud: ") + hipGetErrorString(e));
  }
  h->rs.map_ready();
  if (stats) { stats[0] = n_points; stats[1] = (int64_t)cnt[0]; stats[2] = (int64_t)cnt[1]; stats[3] = occupied; }
  return DIRECT_OK;
}

direct_status_t direct_cluster_get_map(direct_cluster_handle_t h, int32_t mem, uint8_t* map_data) {
  if (!h || !map_data) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  return fetch_resident(h, mem, (size_t)h->D.G, map_data, h->map);
}

namespace {
// map_integrate_scan and map_integrate_scan_evidence: everything both refuse of a scan behind their null check, in the plain call's
// order and by its messages, the DIRECT_ERR_UNSUPPORTED ones included; S->G is the scan's geometry when nothing is refused
direct_status_t scan_refusal(direct_cluster_handle_t h, const direct_map_scan_t* p, int64_t n_points, int32_t mem, const float* xyz, ScanDev* S) {
  const char* why = cloud_refusal(n_points, mem, xyz);
  if (!why && p->mode != DIRECT_SCAN_RESET && p->mode != DIRECT_SCAN_CONTINUE && p->mode != DIRECT_SCAN_ADOPT) why = "unknown mode";
  if (!why && !ms::flags_known(p->flags)) why = "unknown flags";
  if (!why) why = stride_refusal(p->stride);
  if (!why) why = resolution_refusal(p->resolution);
  if (why) return cfail(DIRECT_ERR_INVALID, why);
  if (!std::isfinite(p->max_range) || !(p->max_range > 0.0)) return cfail(DIRECT_ERR_INVALID, "max_range must be finite and positive");
  for (int a = 0; a < 3; a++) {
    if (!std::isfinite(p->map_lower[a]) || !std::isfinite(p->map_upper[a])) return cfail(DIRECT_ERR_INVALID, "map_lower / map_upper must be finite");
    if (p->inflate[a] < 0) return cfail(DIRECT_ERR_INVALID, "inflate must not be negative");
  }
  const Dev& D = h->D;
  ms::Grid& G = S->G;
  G.resolution = p->resolution; G.inv = 1.0 / p->resolution; G.R2 = p->max_range * p->max_range;
  G.size[0] = D.max_x; G.size[1] = D.max_y; G.size[2] = D.max_z;
  for (int a = 0; a < 3; a++) {
    G.lower[a] = p->map_lower[a]; G.origin[a] = p->origin[a];
    G.start[a] = mc::axis_index_drop(p->origin[a], p->map_lower[a], p->map_upper[a], G.inv, G.size[a]);  // -1 for a NaN too
    if (G.start[a] < 0) return cfail(DIRECT_ERR_INVALID, "the origin lies outside the map");
  }
  if (p->mode == DIRECT_SCAN_ADOPT && !h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "DIRECT_SCAN_ADOPT: the handle has no map");
  if (!(p->max_range * G.inv <= (double)ms::kMaxRangeVox)) return cfail(DIRECT_ERR_UNSUPPORTED, "max_range above 4096 voxels");
  for (int a = 0; a < 3; a++)
    if (p->inflate[a] > ms::kMaxInflate) return cfail(DIRECT_ERR_UNSUPPORTED, "inflate above 64 voxels");
  return DIRECT_OK;
}

// ... the bytes DIRECT_SCAN_ADOPT adopts: under DIRECT_UNKNOWN_OCCUPIED the open map where the handle holds one (the closed map
// would turn unknown space into returns), the map otherwise; asked before the state's scan events ...
const uint8_t* scan_adopts(direct_cluster_handle_t h) {
  return h->unknown_policy == DIRECT_UNKNOWN_OCCUPIED && h->rs.has_open_map() ? h->open_map : h->map;
}

// ... what both allocate behind their refusals (the scan grid and its counters, the known grid of a tracked scan, the dilation
// workspace of at least `ws_cells` grids, the open map and its counters under DIRECT_UNKNOWN_OCCUPIED, the cloud on the device) ...
direct_status_t scan_prepare(direct_cluster_handle_t h, const direct_map_scan_t* p, int64_t n_points, int32_t mem, const float* xyz,
                             size_t ws_cells, ScanDev* S) {
  const size_t cells = (size_t)h->D.G;
  if (!h->scan_raw)
    CHIP_TRY(hs::alloc_all(h->allocs, {hs::want(&h->scan_raw, cells), hs::want(&h->scan_cnt, kScanCounters * sizeof(unsigned long long))}));
  const bool track = (p->flags & DIRECT_SCAN_TRACK_KNOWN) != 0;
  if (track && !h->known) CHIP_TRY(hs::alloc_all(h->allocs, {hs::want(&h->known, cells)}));
  if (h->unknown_policy == DIRECT_UNKNOWN_OCCUPIED && !h->open_map)
    CHIP_TRY(hs::alloc_all(h->allocs, {hs::want(&h->open_map, cells), hs::want(&h->close_cnt, kCloseCounters * sizeof(unsigned long long))}));
  S->n = n_points; S->stride = p->stride; S->raw = h->scan_raw; S->cnt = h->scan_cnt; S->known = track ? h->known : nullptr;
  if (p->inflate[1] > 0 || p->inflate[2] > 0) ws_cells = std::max<size_t>(ws_cells, 2);
  if (ws_cells > 0) CHIP_TRY(hs::grow(h->scan_ws, h->stream, ws_cells * cells));
  return cloud_on_device(h, n_points, p->stride, mem, xyz, &S->xyz);
}

// ... and the end of both, behind the kernels that wrote the scan grid: the dilation into the map with its counters, their
// read-back (with `n_more` counters of the caller's own), the table where something changed, the state's events and stats[0..7].
// `e` is what the call's enqueues have come to so far.  ev (null: untimed) are n_ev events, of which the caller has recorded all
// but the last two, behind the inflation and behind the table; ms receives the n_ev - 1 times between them.
direct_status_t scan_finish(direct_cluster_handle_t h, const direct_map_scan_t* p, const char* name, bool had_map, hipError_t e, hipEvent_t* ev,
                            int n_ev, float* ms, int64_t n_points, int64_t* stats, const unsigned long long* more_dev, unsigned long long* more,
                            int n_more) {
  const size_t cells = (size_t)h->D.G;
  const bool track = (p->flags & DIRECT_SCAN_TRACK_KNOWN) != 0;
  auto tick = [&](int k) { return ev ? hipEventRecord(ev[k], h->stream) : hipSuccess; };
  // DIRECT_UNKNOWN_OCCUPIED: the x pass goes into the open map in its non-counting form, and k_scan_close derives the map and counts
  const bool close = h->unknown_policy == DIRECT_UNKNOWN_OCCUPIED;
  if (e == hipSuccess && close) e = hipMemsetAsync(h->close_cnt, 0, kCloseCounters * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) {  // z, then y, through the workspace where they inflate at all; x last, into the map
    DilateDev P = {};
    P.size[0] = h->D.max_x; P.size[1] = h->D.max_y; P.size[2] = h->D.max_z;
    P.G = (long long)cells; P.cnt = h->scan_cnt; P.src = h->scan_raw;
    const int blocks = (int)std::min<long long>(((long long)cells + 255) / 256, kScanMaxBlocks);
    for (int axis = 2; axis >= 0; axis--) {
      if (axis > 0 && p->inflate[axis] == 0) continue;
      P.axis = axis; P.r = p->inflate[axis];
      P.dst = axis == 0 ? (close ? h->open_map : h->map) : (uint8_t*)h->scan_ws.p + (axis == 2 ? 0 : cells);
      P.raw = axis == 0 && !close ? h->scan_raw : nullptr;
      hipLaunchKernelGGL(k_scan_dilate, dim3(blocks), dim3(256), 0, h->stream, P);
      P.src = P.dst;
    }
    if (close) {
      CloseDev Q = {};
      Q.G = (long long)cells; Q.open = h->open_map; Q.known = h->known; Q.raw = h->scan_raw; Q.map = h->map; Q.cnt = h->scan_cnt; Q.more = h->close_cnt;
      const int close_blocks = (int)std::min<long long>((mcl::groups(Q.G) + 255) / 256, kScanMaxBlocks);
      hipLaunchKernelGGL(k_scan_close, dim3(close_blocks), dim3(256), 0, h->stream, Q);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = tick(n_ev - 2);
  unsigned long long cnt[kScanCounters] = {};
  if (e == hipSuccess) e = hipMemcpyAsync(cnt, h->scan_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && n_more > 0) e = hipMemcpyAsync(more, more_dev, n_more * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
  unsigned long long closed[kCloseCounters] = {};
  if (e == hipSuccess && close) e = hipMemcpyAsync(closed, h->close_cnt, sizeof(closed), hipMemcpyDeviceToHost, h->stream);
  e = hs::drain(h->stream, e);
  const bool changed = !had_map || cnt[kScanSet] + cnt[kScanCleared] > 0;
  if (e == hipSuccess && changed) e = rebuild_sat(h);  // nothing changed: the table, the field, the floor tables and the labels stay
  if (e == hipSuccess) e = tick(n_ev - 1);
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  e = hs::drain(h->stream, e);
  if (e == hipSuccess && ev)
    for (int k = 0; k < n_ev - 1 && e == hipSuccess; k++) e = hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
  if (e != hipSuccess) {  // the map and the scan grid have been touched: nothing describes them any more
    h->rs.scan_ended(rs::ScanEnd::failed);
    if (track) h->rs.known_ended(false);
    return cfail(DIRECT_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
  }
  h->rs.scan_ended(changed ? rs::ScanEnd::changed : rs::ScanEnd::unchanged);
  if (track) h->rs.known_ended(true);
  if (close) {
    h->rs.open_map_ready();
    h->close_stats[0] = (int64_t)closed[kCloseClosed]; h->close_stats[1] = (int64_t)closed[kCloseOpenOnes];
  }
  if (stats) {
    stats[0] = n_points; stats[1] = (int64_t)cnt[kScanSkipped]; stats[2] = (int64_t)cnt[kScanTruncated]; stats[3] = (int64_t)cnt[kScanOutside];
    stats[4] = (int64_t)cnt[kScanRawOnes]; stats[5] = (int64_t)cnt[kScanMapOnes]; stats[6] = (int64_t)cnt[kScanSet]; stats[7] = (int64_t)cnt[kScanCleared];
  }
  return DIRECT_OK;
}
}  // namespace

direct_status_t direct_cluster_map_integrate_scan(direct_cluster_handle_t h, const direct_map_scan_t* p, int64_t n_points, int32_t mem,
                                                  const float* xyz, int64_t* stats) {
  if (!h || !p) return cfail(DIRECT_ERR_INVALID, "null argument");
  ScanDev S = {};
  if (const direct_status_t rc = scan_refusal(h, p, n_points, mem, xyz, &S)) return rc;
  if (const char* why = mcl::scan_refusal(h->unknown_policy, p->flags)) return cfail(DIRECT_ERR_INVALID, why);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const size_t cells = (size_t)h->D.G;
  const bool track = (p->flags & DIRECT_SCAN_TRACK_KNOWN) != 0;
  if (h->scan_timing && !h->scan_ev[0])
    for (hipEvent_t& e : h->scan_ev) CHIP_TRY(hipEventCreate(&e));
  if (const direct_status_t rc = scan_prepare(h, p, n_points, mem, xyz, 0, &S)) return rc;
  const bool had_map = h->rs.has_map();
  auto tick = [&](int k) { return h->scan_timing ? hipEventRecord(h->scan_ev[k], h->stream) : hipSuccess; };
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = hipMemsetAsync(h->scan_cnt, 0, kScanCounters * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess && !had_map) e = hipMemsetAsync(h->map, 0, cells, h->stream);  // the bytes "before" of a handle without a map
  if (e == hipSuccess) {
    if (p->mode == DIRECT_SCAN_ADOPT) e = hipMemcpyAsync(h->scan_raw, scan_adopts(h), cells, hipMemcpyDeviceToDevice, h->stream);
    else if (p->mode == DIRECT_SCAN_RESET || !h->rs.has_scan_grid()) e = hipMemsetAsync(h->scan_raw, 0, cells, h->stream);
  }
  if (e == hipSuccess && track && (p->mode == DIRECT_SCAN_RESET || !h->rs.has_known())) e = hipMemsetAsync(h->known, 0, cells, h->stream);
  h->rs.scan_began();  // no scan grid until the call has ended well
  if (track) h->rs.known_scan_began();  // ... and no known grid
  else h->rs.known_dropped();           // the rays of an untracked scan are not recorded: a known grid no longer describes what was seen
  h->rs.evidence_dropped();             // the scan grid is written behind the evidence's back: an evidence grid no longer describes it
  const int ray_blocks = (int)std::min<long long>((n_points + 255) / 256, kScanMaxBlocks);
  if (e == hipSuccess) e = tick(0);
  if (e == hipSuccess && n_points > 0) {
    auto carve = h->scan_test_store ? (track ? k_scan_carve<true, true> : k_scan_carve<true, false>)
                                    : (track ? k_scan_carve<false, true> : k_scan_carve<false, false>);
    hipLaunchKernelGGL(carve, dim3(ray_blocks), dim3(256), 0, h->stream, S);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = tick(1);
  if (e == hipSuccess && n_points > 0) {
    hipLaunchKernelGGL(track ? k_scan_mark<true> : k_scan_mark<false>, dim3(ray_blocks), dim3(256), 0, h->stream, S);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = tick(2);
  return scan_finish(h, p, "map_integrate_scan", had_map, e, h->scan_timing ? h->scan_ev : nullptr, 5, h->scan_ms, n_points, stats, nullptr, nullptr, 0);
}

direct_status_t direct_cluster_map_integrate_scan_evidence(direct_cluster_handle_t h, const direct_map_evidence_t* p, int64_t n_points,
                                                           int32_t mem, const float* xyz, int64_t* stats) {
  if (!h || !p) return cfail(DIRECT_ERR_INVALID, "null argument");
  const direct_map_scan_t* sp = &p->scan;
  ScanDev S = {};
  if (const direct_status_t rc = scan_refusal(h, sp, n_points, mem, xyz, &S)) return rc;
  EvidDev E = {};
  E.P.hit = p->hit; E.P.miss = p->miss; E.P.ev_min = p->ev_min; E.P.ev_max = p->ev_max; E.P.occ = p->occ;
  if (const char* why = me::refusal(E.P, p->reserved)) return cfail(DIRECT_ERR_INVALID, why);
  if (const char* why = mcl::scan_refusal(h->unknown_policy, sp->flags)) return cfail(DIRECT_ERR_INVALID, why);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const size_t cells = (size_t)h->D.G;
  const bool track = (sp->flags & DIRECT_SCAN_TRACK_KNOWN) != 0, adopt = sp->mode == DIRECT_SCAN_ADOPT;
  if (!h->evid) CHIP_TRY(hs::alloc_all(h->allocs, {hs::want(&h->evid, cells), hs::want(&h->evid_cnt, kEvidCounters * sizeof(unsigned long long))}));
  if (h->scan_timing && !h->evid_ev[0])
    for (hipEvent_t& e : h->evid_ev) CHIP_TRY(hipEventCreate(&e));
  if (const direct_status_t rc = scan_prepare(h, sp, n_points, mem, xyz, 1, &S)) return rc;  // the touch grid: the workspace's first grid
  uint8_t* touch = (uint8_t*)h->scan_ws.p;
  E.G = (long long)cells; E.touch = touch; E.ev = h->evid; E.map = adopt ? scan_adopts(h) : nullptr; E.raw = h->scan_raw; E.known = S.known; E.cnt = h->evid_cnt;
  const bool had_map = h->rs.has_map();
  auto tick = [&](int k) { return h->scan_timing ? hipEventRecord(h->evid_ev[k], h->stream) : hipSuccess; };
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = hipMemsetAsync(h->scan_cnt, 0, kScanCounters * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->evid_cnt, 0, kEvidCounters * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(touch, 0, cells, h->stream);
  if (e == hipSuccess && !had_map) e = hipMemsetAsync(h->map, 0, cells, h->stream);  // the bytes "before" of a handle without a map
  // the fold compares before it stores: what it compares with has to be defined.  ADOPT takes the map's bytes and stores always.
  if (e == hipSuccess && !adopt && (sp->mode == DIRECT_SCAN_RESET || !h->rs.has_evidence())) e = hipMemsetAsync(h->evid, 0, cells, h->stream);
  if (e == hipSuccess && !h->rs.has_scan_grid()) e = hipMemsetAsync(h->scan_raw, 0, cells, h->stream);
  if (e == hipSuccess && track && (sp->mode == DIRECT_SCAN_RESET || !h->rs.has_known())) e = hipMemsetAsync(h->known, 0, cells, h->stream);
  h->rs.scan_began();           // no scan grid until the call has ended well
  h->rs.evidence_scan_began();  // ... no evidence grid
  if (track) h->rs.known_scan_began();  // ... and no known grid
  else h->rs.known_dropped();           // the rays of an untracked scan are not recorded, as in the plain call
  const int ray_blocks = (int)std::min<long long>((n_points + 255) / 256, kScanMaxBlocks);
  if (e == hipSuccess) e = tick(0);
  if (e == hipSuccess && n_points > 0) {
    hipLaunchKernelGGL(h->scan_test_store ? k_evid_touch<true> : k_evid_touch<false>, dim3(ray_blocks), dim3(256), 0, h->stream, S, touch);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = tick(1);
  if (e == hipSuccess && n_points > 0) {
    hipLaunchKernelGGL(k_evid_hit, dim3(ray_blocks), dim3(256), 0, h->stream, S, touch);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = tick(2);
  if (e == hipSuccess) {
    const long long groups = ((long long)cells + kEvidGroup - 1) / kEvidGroup;
    const int blocks = (int)std::min<long long>((groups + 255) / 256, kScanMaxBlocks);
    auto fold = adopt ? (track ? k_evid_fold<true, true> : k_evid_fold<true, false>) : (track ? k_evid_fold<false, true> : k_evid_fold<false, false>);
    hipLaunchKernelGGL(fold, dim3(blocks), dim3(256), 0, h->stream, E);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = tick(3);
  unsigned long long more[kEvidCounters] = {};
  const direct_status_t rc = scan_finish(h, sp, "map_integrate_scan_evidence", had_map, e, h->scan_timing ? h->evid_ev : nullptr, 6, h->evid_ms,
                                         n_points, stats, h->evid_cnt, more, kEvidCounters);
  h->rs.evidence_ended(rc == DIRECT_OK);
  h->evid_timed = h->scan_timing && rc == DIRECT_OK;
  if (rc == DIRECT_OK && stats)
    for (int k = 0; k < kEvidCounters; k++) stats[8 + k] = (int64_t)more[k];
  return rc;
}

direct_status_t direct_cluster_get_evidence(direct_cluster_handle_t h, int32_t mem, int8_t* ev) {
  if (!h || !ev) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (!h->rs.has_evidence()) return cfail(DIRECT_ERR_INVALID, "the handle has no evidence grid");
  return fetch_resident(h, mem, (size_t)h->D.G, ev, h->evid);
}

direct_status_t direct_cluster_set_evidence(direct_cluster_handle_t h, int32_t mem, const int8_t* ev) {
  if (!h) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const size_t cells = (size_t)h->D.G;
  if (!h->evid) CHIP_TRY(hs::alloc_all(h->allocs, {hs::want(&h->evid, cells), hs::want(&h->evid_cnt, kEvidCounters * sizeof(unsigned long long))}));
  const int8_t* src = ev;
  if (ev && mem == DIRECT_MEM_HOST) {
    CHIP_TRY(hs::grow(h->known_in, h->stream, cells));  // the staging of set_known's host bytes serves both: each call drains
    src = (const int8_t*)h->known_in.p;
  }
  h->rs.evidence_dropped();  // the grid is about to be written: not present until the call has drained
  hipError_t e = hipSuccess;
  if (!ev) {
    e = hipMemsetAsync(h->evid, 0, cells, h->stream);
  } else {
    if (mem == DIRECT_MEM_HOST) e = hipMemcpyAsync(h->known_in.p, ev, cells, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      const int blocks = (int)std::min<long long>(((long long)cells + 255) / 256, kScanMaxBlocks);
      hipLaunchKernelGGL(k_evid_set, dim3(blocks), dim3(256), 0, h->stream, h->evid, src, (long long)cells);
      e = hipGetLastError();
    }
  }
  e = hs::drain(h->stream, e);
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("set_evidence: ") + hipGetErrorString(e));
  h->rs.evidence_set();
  return DIRECT_OK;
}

direct_status_t direct_cluster_evidence_phase_ms(direct_cluster_handle_t h, float* ms5) {
  if (!h || !ms5) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!h->scan_timing || !h->evid_timed) return cfail(DIRECT_ERR_INVALID, "no timed evidence scan: set DIRECT_CLUSTER_SCAN_TIMING=1 before direct_cluster_create");
  for (int k = 0; k < 5; k++) ms5[k] = h->evid_ms[k];
  return DIRECT_OK;
}

direct_status_t direct_cluster_get_scan_grid(direct_cluster_handle_t h, int32_t mem, uint8_t* raw) {
  if (!h || !raw) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (!h->rs.has_scan_grid()) return cfail(DIRECT_ERR_INVALID, "the handle has no scan grid");
  return fetch_resident(h, mem, (size_t)h->D.G, raw, h->scan_raw);
}

direct_status_t direct_cluster_set_unknown_policy(direct_cluster_handle_t h, int32_t policy) {
  if (!h) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mcl::policy_known(policy)) return cfail(DIRECT_ERR_INVALID, "policy is neither DIRECT_UNKNOWN_FREE nor DIRECT_UNKNOWN_OCCUPIED");
  h->unknown_policy = policy;  // no grid is touched and no map event raised: the next scan derives the map under it
  return DIRECT_OK;
}

direct_status_t direct_cluster_get_unknown_policy(direct_cluster_handle_t h, int32_t* policy, int64_t* stats2) {
  if (!h || !policy) return cfail(DIRECT_ERR_INVALID, "null argument");
  *policy = h->unknown_policy;
  if (stats2)
    for (int k = 0; k < 2; k++) stats2[k] = h->rs.has_open_map() ? h->close_stats[k] : 0;
  return DIRECT_OK;
}

direct_status_t direct_cluster_get_open_map(direct_cluster_handle_t h, int32_t mem, uint8_t* out) {
  if (!h || !out) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (!h->rs.has_open_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no open map");
  return fetch_resident(h, mem, (size_t)h->D.G, out, h->open_map);
}

direct_status_t direct_cluster_scan_phase_ms(direct_cluster_handle_t h, float* ms4) {
  if (!h || !ms4) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!h->scan_timing || !h->rs.has_scan_grid()) return cfail(DIRECT_ERR_INVALID, "no timed scan: set DIRECT_CLUSTER_SCAN_TIMING=1 before direct_cluster_create");
  for (int k = 0; k < 4; k++) ms4[k] = h->scan_ms[k];
  return DIRECT_OK;
}

direct_status_t direct_cluster_polygon_generation_batch(direct_cluster_handle_t h, int32_t batch, const int32_t* seeds,
                                                        int32_t itr_inflate_max, int32_t itr_cluster_max, int32_t mem,
                                                        int32_t* vertex_idx, int32_t* cluster_xyz, int32_t* cluster_num,
                                                        int32_t* cluster_iters, int32_t* rtn) {
  if (!h || !seeds) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (batch <= 0 || batch > h->cfg.max_batch) return cfail(DIRECT_ERR_INVALID, "batch exceeds the handle's max_batch");
  if (itr_inflate_max < 0 || itr_cluster_max < 0) return cfail(DIRECT_ERR_INVALID, "negative iteration limit");
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "direct_cluster_set_map has not been called");
  CHIP_TRY(hipSetDevice(h->cfg.device));
  Dev& D = h->D;
  h->rs.clusters_overwritten();
  CHIP_TRY(hipMemcpyAsync(h->seeds, seeds, (size_t)batch * 3 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  CHIP_TRY(hs::start(h->ev, h->stream));
  int32_t *dv = vertex_idx, *dc = cluster_xyz, *dn = cluster_num, *di = cluster_iters, *dr = rtn;
  if (mem == DIRECT_MEM_HOST) {  // host outputs are staged in buffers the handle owns (allocated once, in create)
    dv = vertex_idx ? h->st_vertex : nullptr; dc = cluster_xyz ? h->st_xyz : nullptr; dn = cluster_num ? h->st_num : nullptr;
    di = cluster_iters ? h->st_iters : nullptr; dr = rtn ? h->st_rtn : nullptr;
  }
  std::vector<Elem> el;
  if (const direct_status_t rc = generation_run(h, batch, h->seeds, itr_inflate_max, itr_cluster_max, dv, dc, dn, di, dr, el)) return rc;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  if (e == hipSuccess && mem == DIRECT_MEM_HOST) {
    auto dn_ = [&](void* dst, const void* src, size_t bytes) {
      return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    };
    if (e == hipSuccess) e = dn_(vertex_idx, dv, (size_t)batch * 24 * 4);
    if (e == hipSuccess && cluster_xyz)  // only the filled prefix of every row
      for (int b = 0; b < batch && e == hipSuccess; b++) {
        const int n = el[b].rtn == DIRECT_CLUSTER_BAD_SEED ? 0 : el[b].n_cluster;
        if (n > 0) e = hipMemcpyAsync(cluster_xyz + (size_t)b * D.ccap * 3, dc + (size_t)b * D.ccap * 3, (size_t)n * 12,
                                      hipMemcpyDeviceToHost, h->stream);
      }
    if (e == hipSuccess) e = dn_(cluster_num, dn, (size_t)batch * 4);
    if (e == hipSuccess) e = dn_(cluster_iters, di, (size_t)batch * 4);
    if (e == hipSuccess) e = dn_(rtn, dr, (size_t)batch * 4);
  }
  e = hs::drain(h->stream, e);
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("polygon_generation_batch: ") + hipGetErrorString(e));
  h->rs.generation_left(batch);
  return DIRECT_OK;
}

direct_status_t direct_cluster_convex_test(direct_cluster_handle_t h, const uint8_t* inside_data, int32_t n_candidate,
                                           const int32_t* candidate_xyz, int32_t n_cluster, const int32_t* cluster_xyz,
                                           uint8_t* can_clu, uint8_t* can_can, uint8_t* accept) {
  if (!h || !inside_data || !candidate_xyz || (!cluster_xyz && n_cluster > 0) || !can_clu)
    return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "direct_cluster_set_map has not been called");
  Dev& D = h->D;
  if (n_candidate <= 0 || n_candidate > D.kcap || n_cluster < 0 || n_cluster > D.ccap)
    return cfail(DIRECT_ERR_INVALID, "candidate / cluster count exceeds the handle's capacity");
  CHIP_TRY(hipSetDevice(h->cfg.device));
  auto pack = [&](const int32_t* xyz, int n, std::vector<int>& out) -> bool {
    out.resize(n);
    for (int i = 0; i < n; i++) {
      const int x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
      if (x < 0 || x >= D.max_x || y < 0 || y >= D.max_y || z < 0 || z >= D.max_z) return false;
      out[i] = (x << 20) | (y << 10) | z;
    }
    return true;
  };
  std::vector<int> pc, pk;
  if (!pack(candidate_xyz, n_candidate, pc) || !pack(cluster_xyz, n_cluster, pk)) return cfail(DIRECT_ERR_INVALID, "voxel outside the map");
  Elem E = {};
  E.n_cluster = n_cluster; E.n_cand = n_candidate; E.live = 1;
  h->rs.clusters_overwritten();  // element 0's cluster, candidates and flags are overwritten below: the last generation's clusters are gone
  CHIP_TRY(hipMemcpyAsync(h->inside_tmp, inside_data, (size_t)D.G, hipMemcpyHostToDevice, h->stream));
  CHIP_TRY(hipMemcpyAsync(D.cand, pc.data(), (size_t)n_candidate * 4, hipMemcpyHostToDevice, h->stream));
  if (n_cluster) CHIP_TRY(hipMemcpyAsync(D.cluster, pk.data(), (size_t)n_cluster * 4, hipMemcpyHostToDevice, h->stream));
  CHIP_TRY(hipMemcpyAsync(D.el, &E, sizeof E, hipMemcpyHostToDevice, h->stream));
  CHIP_TRY(hipMemsetAsync(D.blocked, 0, (size_t)n_candidate * D.kwords * 8, h->stream));
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipLaunchKernelGGL(k_flags_init, dim3(std::min((D.G + 255) / 256, 4096), 1), dim3(256), 0, h->stream, D, (const uint8_t*)h->inside_tmp);
  hipLaunchKernelGGL(k_chunk_box, dim3(D.nchunk, 1), dim3(256), 0, h->stream, D);
  hipLaunchKernelGGL(k_convex<true>, dim3(n_candidate, 1), dim3(256), 0, h->stream, D);
  hipLaunchKernelGGL(k_resolve, dim3(1), dim3(64), (size_t)D.kwords * 8, h->stream, D, 1);
  CHIP_TRY(hipGetLastError());
  CHIP_TRY(hs::stop(h->ev, h->stream));
  std::vector<unsigned long long> rows(can_can ? (size_t)n_candidate * D.kwords : 0);
  CHIP_TRY(hipMemcpyAsync(can_clu, D.can_clu, (size_t)n_candidate, hipMemcpyDeviceToHost, h->stream));
  if (accept) CHIP_TRY(hipMemcpyAsync(accept, D.accept, (size_t)n_candidate, hipMemcpyDeviceToHost, h->stream));
  if (can_can) CHIP_TRY(hipMemcpyAsync(rows.data(), D.blocked, rows.size() * 8, hipMemcpyDeviceToHost, h->stream));
  CHIP_TRY(hipStreamSynchronize(h->stream));
  if (can_can)
    for (int i = 0; i < n_candidate; i++)
      for (int j = 0; j < i; j++)
        can_can[(size_t)i * (i - 1) / 2 + j] = ((rows[(size_t)i * D.kwords + (j >> 6)] >> (j & 63)) & 1ull) ? 0 : 1;
  return DIRECT_OK;
}

direct_status_t direct_cluster_hull_planes_batch(direct_cluster_handle_t h, int32_t batch, int32_t mem_in,
                                                 const int32_t* cluster_xyz, const int32_t* cluster_num, double resolution,
                                                 const double* map_lower, int32_t plane_capacity, int32_t vertex_capacity,
                                                 int32_t mem, double* planes, int64_t* plane_int, int32_t* n_planes,
                                                 double* vertices, int32_t* n_vertices, double* center, int32_t* degenerate,
                                                 int32_t* rtn) {
  if (!h || !map_lower) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (batch <= 0 || batch > h->cfg.max_batch) return cfail(DIRECT_ERR_INVALID, "batch exceeds the handle's max_batch");
  if (cluster_xyz && !cluster_num) return cfail(DIRECT_ERR_INVALID, "cluster_xyz without cluster_num");
  if (plane_capacity <= 0 || vertex_capacity <= 0 || !(resolution > 0)) return cfail(DIRECT_ERR_INVALID, "bad capacity / resolution");
  if (!cluster_xyz && batch > h->rs.clusters_resident())
    return cfail(DIRECT_ERR_INVALID, "no resident clusters for this batch: call direct_cluster_polygon_generation_batch with at least "
                                     "`batch` seeds first (caller-provided voxels replace the resident clusters)");
  if (cluster_xyz) h->rs.clusters_overwritten();  // the voxels are packed into the handle's cluster storage: the generation's clusters are gone
  CHIP_TRY(hipSetDevice(h->cfg.device));
  Dev& D = h->D;
  if (const direct_status_t rc = hull_workspace(h)) return rc;
  // device views of the outputs: the caller's pointers, or slices of one staging block for host outputs (nothing is filled:
  // the host arrays hold what the block held wherever k_hull_finish does not write)
  const size_t nb = (size_t)batch;
  const size_t sz[8] = {nb * plane_capacity * 4 * sizeof(double), nb * plane_capacity * 4 * sizeof(long long), nb * sizeof(int32_t),
                        nb * vertex_capacity * 3 * sizeof(double), nb * sizeof(int32_t), nb * 3 * sizeof(double),
                        nb * sizeof(int32_t), nb * sizeof(int32_t)};
  void* const user[8] = {planes, plane_int, n_planes, vertices, n_vertices, center, degenerate, rtn};
  void* dev[8];
  hs::Stage st(mem == DIRECT_MEM_HOST);
  for (int i = 0; i < 8; i++) hs::stage_out(st, &dev[i], user[i], sz[i]);
  CHIP_TRY(hs::stage_upload(st, h->hull_out, h->stream));
  const int32_t *sx = cluster_xyz, *sn = cluster_num;
  if (cluster_xyz && mem_in == DIRECT_MEM_HOST) {  // caller-provided voxels from the host: the filled prefix of every row,
                                                   // through the generation's own staging blocks (st_xyz, st_num)
    for (int b = 0; b < batch; b++) {
      const int n = cluster_num[b] < 0 ? 0 : (cluster_num[b] > D.ccap ? D.ccap : cluster_num[b]);
      if (n > 0)
        CHIP_TRY(hipMemcpyAsync(h->st_xyz + (size_t)b * D.ccap * 3, cluster_xyz + (size_t)b * D.ccap * 3, (size_t)n * 12,
                                hipMemcpyHostToDevice, h->stream));
    }
    CHIP_TRY(hipMemcpyAsync(h->st_num, cluster_num, nb * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    sx = h->st_xyz; sn = h->st_num;
  }
  CHIP_TRY(hs::start(h->ev, h->stream));
  if (const direct_status_t rc = hull_run(h, batch, sx, sn, resolution, map_lower, plane_capacity, vertex_capacity, dev)) return rc;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  e = hs::drain(h->stream, hs::stage_download(st, h->stream, e));
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("hull_planes_batch: ") + hipGetErrorString(e));
  return DIRECT_OK;
}

direct_status_t direct_cluster_grid_path_batch(direct_cluster_handle_t h, int32_t batch, const int32_t* starts, const int32_t* goals,
                                               int32_t path_capacity, int32_t max_rounds, int32_t mem, int32_t* path_xyz,
                                               int32_t* path_len, double* path_cost, double* dist, int32_t* stats, int32_t* rtn) {
  if (!h || !starts || !goals) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (batch <= 0 || batch > h->cfg.max_batch) return cfail(DIRECT_ERR_INVALID, "batch exceeds the handle's max_batch");
  if (path_capacity <= 0 || max_rounds < 0) return cfail(DIRECT_ERR_INVALID, "path_capacity must be positive, max_rounds not negative");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "direct_cluster_set_map has not been called");
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const PathCall call = {"grid_path_batch", batch, batch, path_capacity, max_rounds, mem, starts, goals, false, 0, 0, nullptr, dist};
  void* const user[7] = {path_xyz, path_len, path_cost, stats, rtn, nullptr, nullptr};
  void* dev[7];
  hs::Stage st(mem == DIRECT_MEM_HOST);
  return grid_path_run(h, call, st, [&](PathDev& P, PathClearDev& C) { return path_pair_stage(h, call, st, P, C, user, dev); },
                       [&](const PathDev& P, const PathClearDev&, int r) {
                         hipLaunchKernelGGL(k_path_relax, dim3(P.ntiles, batch), dim3(256), 0, h->stream, P, r);
                       },
                       [&](const PathDev& P, const PathClearDev&, int done) {
                         hipLaunchKernelGGL(k_path_trace, dim3(batch), dim3(64), 0, h->stream, P, done, (int32_t*)dev[0], (int32_t*)dev[1],
                                            (double*)dev[2], (int32_t*)dev[3], (int32_t*)dev[4]);
                       });
}

direct_status_t direct_cluster_plan_check_batch(direct_cluster_handle_t h, const direct_plan_check_in_t* in, direct_plan_check_out_t* out) {
  const char* why = plan_rows_refusal(h, in, out);
  if (!why && in->outside_blocks != 0 && in->outside_blocks != 1) why = "outside_blocks is neither 0 nor 1";
  if (!why) why = plan_map_refusal(h, in, in->margin, "margin must be finite and not negative");
  if (why) return cfail(DIRECT_ERR_INVALID, why);
  // host arrays go through one staging block: n_seg, T, coef, t_from in; the six outputs back, of which seg_first alone is
  // filled (0xff: entries past n_seg read -1)
  hs::Stage st(in->mem == DIRECT_MEM_HOST);
  PlanDev A = {};
  if (const direct_status_t rc = plan_rows_stage(h, st, in, A.R, A.G)) return rc;
  const size_t B = (size_t)in->batch, slots = B * (size_t)in->n_seg_max;
  // workspace: counters, S, per-slot leaves, unresolved list
  const size_t w_S = up256(256), w_first = w_S + up256((B + slots) * sizeof(double)), w_list = w_first + up256(slots * sizeof(int));
  CHIP_TRY(hs::grow(h->plan_ws, h->stream, w_list + up256(slots * sizeof(int))));
  A.G.margin = in->margin;
  A.G.outside_blocks = in->outside_blocks;
  A.count = out->stats != nullptr;
  char* W = (char*)h->plan_ws.p;
  A.n_list = (unsigned*)W; A.n_tests = (unsigned long long*)(W + 8);
  A.R.S = (double*)(W + w_S); A.ws_first = (int*)(W + w_first); A.list = (int*)(W + w_list);
  hs::stage_out(st, &A.status, out->status, B * 4);
  hs::stage_out(st, &A.verdict, out->verdict, B * 4);
  hs::stage_out(st, &A.t_free, out->t_free, B * 8);
  hs::stage_out(st, &A.first, out->first, B * 8);
  hs::stage_out(st, &A.hit_box, out->hit_box, B * 24);
  hs::stage_out(st, &A.seg_first, out->seg_first, slots * 4, 0xff);
  CHIP_TRY(hs::stage_upload(st, h->plan_io, h->stream));
  unsigned long long cnt[2] = {0, 0};
  const direct_status_t rc = plan_run(h, st, "plan_check_batch: ", [&] {
    const hipError_t e = hipMemsetAsync(W, 0, 16, h->stream);
    if (e != hipSuccess) return e;
    return in->dtype == DIRECT_F32 ? plan_check_launch<float>(h->D, A, h->stream) : plan_check_launch<double>(h->D, A, h->stream);
  }, [&] { return out->stats ? hipMemcpyAsync(cnt, W, sizeof(cnt), hipMemcpyDeviceToHost, h->stream) : hipSuccess; });
  if (rc == DIRECT_OK && out->stats) { out->stats[0] = (int64_t)(cnt[0] & 0xffffffffull); out->stats[1] = (int64_t)cnt[1]; }
  return rc;
}

direct_status_t direct_cluster_distance_field(direct_cluster_handle_t h, int32_t cap_vox, int64_t* stats) {
  if (!h) return cfail(DIRECT_ERR_INVALID, "null argument");
  h->rs.field_call_began();  // every call: labels of free_components built with a floor no longer count as describing the field
  if (cap_vox < 0 || cap_vox > df::kMaxCap) return cfail(DIRECT_ERR_INVALID, "cap_vox outside [0, 1024]");
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const Dev& D = h->D;
  if (!h->dist[0]) {  // all or nothing
    const hipError_t ae = hs::alloc_all(h->allocs, {hs::want(&h->dist[0], (size_t)D.G * sizeof(int32_t)), hs::want(&h->dist[1], (size_t)D.G * sizeof(int32_t)),
                                                    hs::want(&h->dist_cnt, 2 * sizeof(unsigned long long))});
    if (ae != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("distance_field: allocation: ") + hipGetErrorString(ae));
  }
  h->rs.field_build_began();
  DistDev A = {};
  A.map = h->map; A.a = h->dist[0]; A.b = h->dist[1];
  A.X = D.max_x; A.Y = D.max_y; A.Z = D.max_z; A.G = D.G; A.cap2 = df::cap2_of(cap_vox);
  A.cnt = h->dist_cnt;
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = hipMemsetAsync(h->dist_cnt, 0, sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->dist_cnt + 1, 0xff, sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = dist_field_launch(A, stats != nullptr, h->stream);
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  unsigned long long cnt[2] = {0, 0};
  if (e == hipSuccess && stats) e = hipMemcpyAsync(cnt, h->dist_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream);
  e = hs::drain(h->stream, e);
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("distance_field: ") + hipGetErrorString(e));
  h->rs.field_built(A.cap2);
  if (stats) { stats[0] = (int64_t)cnt[0]; stats[1] = (int64_t)(int32_t)(cnt[1] & 0xffffffffull); }
  return DIRECT_OK;
}

direct_status_t direct_cluster_get_distance_field(direct_cluster_handle_t h, int32_t mem, int32_t* d2) {
  if (!h || !d2) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  if (const char* why = h->rs.field_refusal(0, 0)) return cfail(DIRECT_ERR_INVALID, why);
  return fetch_resident(h, mem, (size_t)h->D.G * sizeof(int32_t), d2, h->dist[0]);
}

direct_status_t direct_cluster_plan_clearance_batch(direct_cluster_handle_t h, const direct_plan_clear_in_t* in, direct_plan_clear_out_t* out) {
  const char* why = plan_rows_refusal(h, in, out);
  if (!why) why = plan_map_refusal(h, in, in->radius, "radius must be finite and not negative");
  if (!why) why = h->rs.field_refusal(0, 0);
  if (why) return cfail(DIRECT_ERR_INVALID, why);
  // host arrays go through one staging block of the call's own; seg_clearance alone is filled (0xff: entries past n_seg read NaN)
  hs::Stage st(in->mem == DIRECT_MEM_HOST);
  ClearDev A = {};
  if (const direct_status_t rc = plan_rows_stage(h, st, in, A.R, A.G)) return rc;
  const size_t B = (size_t)in->batch, slots = B * (size_t)in->n_seg_max;
  // workspace: S, then per slot the minimum, its leaf, the first leaf below the radius
  const size_t w_min = up256((B + slots) * sizeof(double)), w_leaf = w_min + up256(slots * sizeof(double)), w_below = w_leaf + up256(slots * sizeof(int));
  CHIP_TRY(hs::grow(h->clear_ws, h->stream, w_below + up256(slots * sizeof(int))));
  char* W = (char*)h->clear_ws.p;
  A.G.resolution = in->resolution;
  A.radius = in->radius;
  A.field = h->dist[0]; A.YZ = h->D.max_yz; A.Z = h->D.max_z;
  A.R.S = (double*)W; A.ws_min = (double*)(W + w_min); A.ws_leaf = (int*)(W + w_leaf); A.ws_below = (int*)(W + w_below);
  hs::stage_out(st, &A.status, out->status, B * 4);
  hs::stage_out(st, &A.clearance, out->clearance, B * 8);
  hs::stage_out(st, &A.where, out->where, B * 8);
  hs::stage_out(st, &A.t_min, out->t_min, B * 8);
  hs::stage_out(st, &A.verdict, out->verdict, B * 4);
  hs::stage_out(st, &A.t_free, out->t_free, B * 8);
  hs::stage_out(st, &A.seg_clearance, out->seg_clearance, slots * 8, 0xff);
  CHIP_TRY(hs::stage_upload(st, h->clear_io, h->stream));
  return plan_run(h, st, "plan_clearance_batch: ",
                  [&] { return in->dtype == DIRECT_F32 ? plan_clear_launch<float>(A, h->stream) : plan_clear_launch<double>(A, h->stream); },
                  [] { return hipSuccess; });
}

direct_status_t direct_cluster_cube_corridor_batch(direct_cluster_handle_t h, const direct_cube_corridor_in_t* in, direct_cube_corridor_out_t* out) {
  if (const direct_status_t rc = cube_corridor_refusal(h, in, out, nullptr)) return rc;
  CHIP_TRY(hipSetDevice(h->cfg.device));
  return cube_corridor_run(h, in, out, h->D, "cube_corridor_batch: ", [] { return hipSuccess; }, [] { return hipSuccess; });
}

direct_status_t direct_cluster_cube_corridor_clear_batch(direct_cluster_handle_t h, const direct_cube_corridor_in_t* in, int32_t min_d2,
                                                         direct_cube_corridor_out_t* out, int64_t* info) {
  if (const direct_status_t rc = cube_corridor_refusal(h, in, out, min_d2 < 0 ? "min_d2 must not be negative" : nullptr)) return rc;
  const bool neutral = cc::floor_neutral(min_d2);  // the map's own table: the field is not looked at
  if (!neutral)
    if (const char* why = h->rs.field_refusal(min_d2, 0)) return cfail(DIRECT_ERR_INVALID, why);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  Dev D = h->D;
  const size_t entries = (size_t)(D.max_x + 1) * D.sat_yz;
  int slot = -1, hit = 1;
  if (!neutral) {
    if (!h->floor_tab[0]) {  // all or nothing
      const hipError_t ae = hs::alloc_all(h->allocs, {hs::want(&h->floor_tab[0], entries * sizeof(int)), hs::want(&h->floor_tab[1], entries * sizeof(int))});
      if (ae != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("cube_corridor_clear_batch: table allocation: ") + hipGetErrorString(ae));
    }
    slot = h->rs.floor_chosen(min_d2, &hit);  // a miss: the slot holds nothing until its build has drained without an error
    D.sat = h->floor_tab[slot];
  }
  int count = 0;  // the table's last entry is the sum over the whole map
  const bool fetch = neutral ? info != nullptr : !hit;
  const direct_status_t rc = cube_corridor_run(h, in, out, D, "cube_corridor_clear_batch: ", [&] {
    if (hit) return hipSuccess;
    hipLaunchKernelGGL(k_floor_fill, dim3((unsigned)std::min<size_t>((entries + 255) / 256, 1024)), dim3(256), 0, h->stream, D, h->dist[0], min_d2);
    for (int axis = 2; axis >= 0; axis--) hipLaunchKernelGGL(k_sat_scan, dim3(256), dim3(256), 0, h->stream, D, axis);
    return hipGetLastError();
  }, [&] { return fetch ? hipMemcpyAsync(&count, D.sat + (entries - 1), sizeof(int), hipMemcpyDeviceToHost, h->stream) : hipSuccess; });
  if (rc != DIRECT_OK) {
    if (!hit) h->rs.floor_build_failed(slot);
    return rc;
  }
  if (!neutral) {
    if (!hit) h->rs.floor_built(slot, min_d2, count);
    h->rs.floor_used(slot);
  }
  if (info) { info[0] = hit ? 0 : 1; info[1] = neutral ? count : h->rs.floor_count(slot); }
  return DIRECT_OK;
}

direct_status_t direct_cluster_corridor_batch(direct_cluster_handle_t h, const direct_cluster_corridor_in_t* in, direct_cluster_corridor_out_t* out,
                                              int64_t* stats) {
  if (const direct_status_t rc = cube_corridor_refusal(h, in, out, in && in->itr_cluster_max < 0 ? "itr_cluster_max must not be negative" : nullptr))
    return rc;
  CHIP_TRY(hipSetDevice(h->cfg.device));
  h->rs.clusters_overwritten();  // the chunks' generations run in the handle's cluster storage: the last generation's clusters are gone
  if (const direct_status_t rc = hull_workspace(h)) return rc;
  const Dev& D = h->D;
  const size_t B = (size_t)in->batch, slots = B * (size_t)in->path_capacity, segs = B * (size_t)in->seg_capacity;
  const size_t P = (size_t)in->p_max, MB = (size_t)h->cfg.max_batch;
  const size_t r = in->plane_dtype == DIRECT_F32 ? sizeof(float) : sizeof(double);
  CorrDev A = {};
  A.batch = in->batch; A.path_cap = in->path_capacity; A.seg_cap = in->seg_capacity; A.p_max = in->p_max; A.pop_back = in->pop_back ? 1 : 0;
  A.X = D.max_x; A.Y = D.max_y; A.Z = D.max_z;
  A.res = in->resolution;
  for (int a = 0; a < 3; a++) A.lower[a] = in->map_lower[a];
  hs::Stage ws(false), si(in->mem_in == DIRECT_MEM_HOST), so(out->mem == DIRECT_MEM_HOST);
  hs::stage_scratch(ws, &A.rows, B * sizeof(kc::Row));
  hs::stage_scratch(ws, &A.st_planes, segs * P * 4 * sizeof(double));
  hs::stage_scratch(ws, &A.st_np, segs * sizeof(int32_t));
  hs::stage_scratch(ws, &A.st_seeds, segs * 3 * sizeof(double));
  hs::stage_scratch(ws, &A.st_centers, segs * 3 * sizeof(double));
  hs::stage_scratch(ws, &A.table, (size_t)D.G * sizeof(int));
  hs::stage_scratch(ws, &A.seed_list, B * 3 * sizeof(int32_t));
  hs::stage_scratch(ws, &A.cnt, 4 * sizeof(unsigned long long));
  hs::stage_scratch(ws, &A.h_planes, MB * P * 4 * sizeof(double));
  hs::stage_scratch(ws, &A.h_np, MB * sizeof(int32_t));
  hs::stage_scratch(ws, &A.h_center, MB * 3 * sizeof(double));
  hs::stage_scratch(ws, &A.h_rtn, MB * sizeof(int32_t));
  hs::stage_in(si, &A.path_xyz, in->path_xyz, slots * 3 * sizeof(int32_t));
  hs::stage_in(si, &A.path_len, in->path_len, B * sizeof(int32_t));
  hs::stage_out(so, &A.n_seg, out->n_seg, B * sizeof(int32_t));
  hs::stage_out(so, &A.n_planes, out->n_planes, segs * sizeof(int32_t));
  hs::stage_out(so, &A.planes, out->planes, segs * P * 4 * r);
  hs::stage_out(so, &A.seeds, out->seeds, segs * 3 * r);
  hs::stage_out(so, &A.centers, out->centers, segs * 3 * r);
  hs::stage_out(so, &A.rtn, out->rtn, B * sizeof(int32_t));
  CHIP_TRY(hs::stage_upload(ws, h->corr_ws, h->stream));
  CHIP_TRY(hs::stage_upload(si, h->corr_in, h->stream));
  CHIP_TRY(hs::stage_upload(so, h->corr_out, h->stream));
  // the owner table starts every call untouched (a call that failed half way may have left entries behind); rounds reset what they touch
  CHIP_TRY(hipMemsetAsync(A.table, 0x7f, (size_t)D.G * sizeof(int), h->stream));
  CHIP_TRY(hipMemsetAsync(A.cnt, 0, 4 * sizeof(unsigned long long), h->stream));
  CHIP_TRY(hs::start(h->ev, h->stream));
  void* const hull_out[8] = {A.h_planes, nullptr, A.h_np, nullptr, nullptr, A.h_center, nullptr, A.h_rtn};
  unsigned long long cnt[4] = {0, 0, 0, 0};
  std::vector<Elem> el;
  long long rounds = 0;
  bool ended = false;
  // Every unfinished row either ends or consumes a point per round, and a row has at most path_capacity points: round
  // path_capacity (counted from 0) finds nothing due.  A loop that gets past it reports DIRECT_ERR_DEVICE.
  for (int round = 0; round <= in->path_capacity && !ended; round++) {
    hipLaunchKernelGGL(k_corr_advance, dim3(in->batch), dim3(64), 0, h->stream, A, round == 0 ? 1 : 0);
    hipLaunchKernelGGL(k_corr_unique, dim3(1), dim3(1024), 0, h->stream, A);
    CHIP_TRY(hipGetLastError());
    CHIP_TRY(hipMemcpyAsync(cnt, A.cnt, sizeof cnt, hipMemcpyDeviceToHost, h->stream));  // the round's one small word
    CHIP_TRY(hipStreamSynchronize(h->stream));
    if (cnt[0] == 0) {
      ended = true;
      break;
    }
    rounds++;
    for (size_t lo = 0; lo < cnt[0]; lo += MB) {
      const int nb = (int)std::min<size_t>(MB, cnt[0] - lo);
      if (const direct_status_t rc = generation_run(h, nb, A.seed_list + 3 * lo, in->itr_inflate_max, in->itr_cluster_max, nullptr, nullptr,
                                                    nullptr, nullptr, nullptr, el))
        return rc;
      if (const direct_status_t rc = hull_run(h, nb, nullptr, nullptr, in->resolution, in->map_lower, in->p_max, 1, hull_out)) return rc;
      hipLaunchKernelGGL(k_corr_append, dim3(in->batch), dim3(64), 0, h->stream, D, A, (int)lo, nb);
      CHIP_TRY(hipGetLastError());
    }
  }
  if (!ended) {
    (void)hipStreamSynchronize(h->stream);
    return cfail(DIRECT_ERR_DEVICE, "corridor_batch: rows still walking after path_capacity + 1 rounds");
  }
  if (in->plane_dtype == DIRECT_F32) hipLaunchKernelGGL(k_corr_emit<float>, dim3(in->batch), dim3(256), 0, h->stream, A);
  else hipLaunchKernelGGL(k_corr_emit<double>, dim3(in->batch), dim3(256), 0, h->stream, A);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  e = hs::drain(h->stream, hs::stage_download(so, h->stream, e));
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("corridor_batch: ") + hipGetErrorString(e));
  if (stats) { stats[0] = rounds; stats[1] = (int64_t)cnt[1]; stats[2] = (int64_t)cnt[2]; stats[3] = (int64_t)cnt[3]; }
  return DIRECT_OK;
}

direct_status_t direct_cluster_grid_path_clear_batch(direct_cluster_handle_t h, const direct_grid_path_clear_in_t* in,
                                                     direct_grid_path_clear_out_t* out) {
  if (!h || !in || !out || !in->starts || !in->goals) return cfail(DIRECT_ERR_INVALID, "null argument");
  // what the arguments alone decide comes first, then what the handle holds
  if (in->batch <= 0) return cfail(DIRECT_ERR_INVALID, "batch must be positive");
  if (in->path_capacity <= 0 || in->max_rounds < 0) return cfail(DIRECT_ERR_INVALID, "path_capacity must be positive, max_rounds not negative");
  if (!mem_kind(in->mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (const char* why = clear_args_refusal(in->min_d2, in->n_penalty, in->penalty)) return cfail(DIRECT_ERR_INVALID, why);
  if (in->batch > h->cfg.max_batch) return cfail(DIRECT_ERR_INVALID, "batch exceeds the handle's max_batch");
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  if (const char* why = h->rs.field_refusal(in->min_d2, in->n_penalty)) return cfail(DIRECT_ERR_INVALID, why);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const int batch = in->batch;
  const PathCall call = {"grid_path_clear_batch", batch, batch, in->path_capacity, in->max_rounds, in->mem, in->starts, in->goals, true,
                         in->min_d2, in->n_penalty, in->penalty, out->dist};
  void* const user[7] = {out->path_xyz, out->path_len, out->path_cost, out->stats, out->rtn, out->path_d2, out->path_min_d2};
  void* dev[7];
  hs::Stage st(in->mem == DIRECT_MEM_HOST);
  return grid_path_run(h, call, st, [&](PathDev& P, PathClearDev& C) { return path_pair_stage(h, call, st, P, C, user, dev); },
                       [&](const PathDev& P, const PathClearDev& C, int r) {
                         hipLaunchKernelGGL(k_path_clear_relax, dim3(P.ntiles, batch), dim3(256), 0, h->stream, P, C, r);
                       },
                       [&](const PathDev& P, const PathClearDev& C, int done) {
                         hipLaunchKernelGGL(k_path_clear_trace, dim3(batch), dim3(64), 0, h->stream, P, C, done, (int32_t*)dev[0], (int32_t*)dev[1],
                                            (double*)dev[2], (int32_t*)dev[3], (int32_t*)dev[4], (int32_t*)dev[5], (int32_t*)dev[6]);
                       });
}

direct_status_t direct_cluster_grid_path_fan_batch(direct_cluster_handle_t h, const direct_grid_path_fan_in_t* in,
                                                   direct_grid_path_fan_out_t* out) {
  if (!h || !in || !out || !in->sources || !in->goals) return cfail(DIRECT_ERR_INVALID, "null argument");
  // what the arguments alone decide comes first, then what the handle holds
  if (in->n_src < 1) return cfail(DIRECT_ERR_INVALID, "n_src must be positive");
  if (in->n_goal < 1) return cfail(DIRECT_ERR_INVALID, "n_goal must be positive");
  if (in->path_capacity <= 0 || in->max_rounds < 0) return cfail(DIRECT_ERR_INVALID, "path_capacity must be positive, max_rounds not negative");
  if (!mem_kind(in->mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (const char* why = clear_args_refusal(in->min_d2, in->n_penalty, in->penalty)) return cfail(DIRECT_ERR_INVALID, why);
  if (!in->goal_src && in->n_src != 1) return cfail(DIRECT_ERR_INVALID, "a NULL goal_src requires n_src == 1");
  if (in->goal_src)
    for (int j = 0; j < in->n_goal; j++)
      if (in->goal_src[j] < 0 || in->goal_src[j] >= in->n_src) return cfail(DIRECT_ERR_INVALID, "goal_src entry outside [0, n_src)");
  const bool clear = !(in->min_d2 <= 1 && in->n_penalty == 0);
  if (!clear && (out->path_d2 || out->path_min_d2))
    return cfail(DIRECT_ERR_INVALID, "path_d2 and path_min_d2 must be NULL in neutral mode (min_d2 <= 1, n_penalty == 0)");
  if (in->n_src > h->cfg.max_batch) return cfail(DIRECT_ERR_INVALID, "n_src exceeds the handle's max_batch");
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  if (clear)
    if (const char* why = h->rs.field_refusal(in->min_d2, in->n_penalty)) return cfail(DIRECT_ERR_INVALID, why);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  // k_path_init's (start, goal) of a field = (source, source)
  const PathCall call = {"grid_path_fan_batch", in->n_src, in->n_goal, in->path_capacity, in->max_rounds, in->mem, in->sources, in->sources, clear,
                         in->min_d2, in->n_penalty, in->penalty, out->dist};
  const size_t ns = (size_t)in->n_src, ng = (size_t)in->n_goal, cap = (size_t)in->path_capacity;
  // the goals, their sources and the grouping by source (a counting sort: the goals of a source in the caller's order), one array
  std::vector<int> meta(3 * ng + ng + ng + ns + 1);
  int *m_goal = meta.data(), *m_src = m_goal + 3 * ng, *m_order = m_src + ng, *m_off = m_order + ng;
  std::copy(in->goals, in->goals + 3 * ng, m_goal);
  for (size_t j = 0; j < ng; j++) m_src[j] = in->goal_src ? in->goal_src[j] : 0;
  std::fill(m_off, m_off + ns + 1, 0);
  for (size_t j = 0; j < ng; j++) m_off[m_src[j] + 1]++;
  for (size_t s = 0; s < ns; s++) m_off[s + 1] += m_off[s];
  {
    std::vector<int> at(m_off, m_off + ns);
    for (size_t j = 0; j < ng; j++) m_order[at[m_src[j]]++] = (int)j;
  }
  // Two blocks, both or neither: the workspace (host inputs and scratch, whatever `mem` is) and the staging of host outputs.
  FanDev F = {};
  F.n_src = in->n_src; F.n_goal = in->n_goal;
  int* d_meta = nullptr;
  hs::Stage sw(true), so(in->mem == DIRECT_MEM_HOST);
  hs::stage_in(sw, &d_meta, meta.data(), meta.size() * sizeof(int));
  hs::stage_scratch(sw, &F.bound, ns * sizeof(double));
  hs::stage_scratch(sw, &F.ring, out->path_xyz ? ng * cap * sizeof(int) : 0);
  hs::stage_scratch(sw, &F.ring_d2, out->path_d2 ? ng * cap * sizeof(int) : 0);
  const size_t sz[7] = {ng * cap * 3 * sizeof(int32_t), ng * sizeof(int32_t), ng * sizeof(double), ng * sizeof(int32_t),
                        ng * cap * sizeof(int32_t), ng * sizeof(int32_t), ns * 2 * sizeof(int32_t)};
  void* const user[7] = {out->path_xyz, out->path_len, out->path_cost, out->rtn, out->path_d2, out->path_min_d2, out->stats};
  void* dev[7];
  for (int i = 0; i < 7; i++) hs::stage_out(so, &dev[i], user[i], sz[i]);
  return grid_path_run(h, call, so, [&](PathDev&, PathClearDev&) -> direct_status_t {
    hipError_t ue = hs::stage_upload(sw, h->fan_ws, h->stream);
    if (ue == hipSuccess) ue = hs::stage_upload(so, h->fan_out, h->stream);
    if (ue != hipSuccess) {
      (void)hipStreamSynchronize(h->stream);
      hs::release(h->fan_ws);
      hs::release(h->fan_out);
      return cfail(DIRECT_ERR_DEVICE, std::string("grid_path_fan_batch: workspace allocation: ") + hipGetErrorString(ue));
    }
    F.goals = d_meta; F.gsrc = d_meta + 3 * ng; F.order = F.gsrc + ng; F.off = F.order + ng;
    return DIRECT_OK;
  }, [&](const PathDev& P, const PathClearDev& C, int r) {
    // k_fan_bound goes in front of every round, or of every batch of rounds (fan_bound_every: 1 or gp::kFanRoundsPerCheck, and a
    // batch starts at a multiple of that)
    const dim3 tiles(P.ntiles, in->n_src);
    const bool bound = r % h->fan_bound_every == 0;
    if (clear) {
      if (bound) hipLaunchKernelGGL(k_fan_bound<true>, dim3(F.n_src), dim3(kFanBoundLanes), 0, h->stream, P, C, F);
      hipLaunchKernelGGL(k_fan_relax<true>, tiles, dim3(256), 0, h->stream, P, C, (const double*)F.bound, r);
    } else {
      if (bound) hipLaunchKernelGGL(k_fan_bound<false>, dim3(F.n_src), dim3(kFanBoundLanes), 0, h->stream, P, C, F);
      hipLaunchKernelGGL(k_fan_relax<false>, tiles, dim3(256), 0, h->stream, P, C, (const double*)F.bound, r);
    }
  }, [&](const PathDev& P, const PathClearDev& C, int done) {
    if (clear)
      hipLaunchKernelGGL(k_fan_trace<true>, dim3(in->n_goal), dim3(64), 0, h->stream, P, C, F, done, (int32_t*)dev[0], (int32_t*)dev[1],
                         (double*)dev[2], (int32_t*)dev[3], (int32_t*)dev[4], (int32_t*)dev[5]);
    else
      hipLaunchKernelGGL(k_fan_trace<false>, dim3(in->n_goal), dim3(64), 0, h->stream, P, C, F, done, (int32_t*)dev[0], (int32_t*)dev[1],
                         (double*)dev[2], (int32_t*)dev[3], (int32_t*)nullptr, (int32_t*)nullptr);
    if (dev[6]) hipLaunchKernelGGL(k_fan_stats, dim3(1), dim3(64), 0, h->stream, P, in->n_src, (int32_t*)dev[6]);
  });
}

direct_status_t direct_cluster_free_components(direct_cluster_handle_t h, int32_t min_d2, int64_t* stats) {
  if (!h) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (min_d2 < 0) return cfail(DIRECT_ERR_INVALID, "min_d2 must not be negative");
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  const int32_t floor = fc::normal_floor(min_d2);
  if (floor)
    if (const char* why = h->rs.field_refusal(floor, 0)) return cfail(DIRECT_ERR_INVALID, why);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const Dev& D = h->D;
  if (!h->comp_label) {  // all or nothing
    const hipError_t ae = hs::alloc_all(h->allocs, {hs::want(&h->comp_label, (size_t)D.G * sizeof(int32_t)), hs::want(&h->comp_size, (size_t)D.G * sizeof(int32_t)),
                                                    hs::want(&h->comp_cnt, 4 * sizeof(unsigned long long))});
    if (ae != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("free_components: allocation: ") + hipGetErrorString(ae));
  }
  h->rs.label_build_began();
  CompDev A = {};
  A.map = h->map; A.d2 = floor ? h->dist[0] : nullptr; A.label = h->comp_label; A.size = h->comp_size; A.cnt = h->comp_cnt;
  A.X = D.max_x; A.Y = D.max_y; A.Z = D.max_z; A.G = D.G; A.min_d2 = floor;
  A.tx = gp::tiles_along(A.X); A.ty = gp::tiles_along(A.Y); A.tz = gp::tiles_along(A.Z);
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = hipMemsetAsync(h->comp_cnt, 0, 4 * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->comp_size, 0, (size_t)D.G * sizeof(int32_t), h->stream);
  if (e == hipSuccess) e = free_comp_launch(A, h->stream);
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  unsigned long long cnt[4] = {0, 0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(cnt, h->comp_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream);
  e = hs::drain(h->stream, e);
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("free_components: ") + hipGetErrorString(e));
  if (cnt[3]) return cfail(DIRECT_ERR_DEVICE, "free_components: a union-find loop passed its trip bound (error word " + std::to_string(cnt[3]) + ")");
  h->rs.labels_built(floor);
  if (stats) { stats[0] = (int64_t)cnt[0]; stats[1] = (int64_t)cnt[1]; stats[2] = fc::stat_size(cnt[2]); stats[3] = fc::stat_label(cnt[2]); }
  return DIRECT_OK;
}

direct_status_t direct_cluster_get_free_components(direct_cluster_handle_t h, int32_t mem, int32_t* label, int32_t* size, int32_t* min_d2_built) {
  if (!h) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  if (!h->rs.labels_serve()) return cfail(DIRECT_ERR_INVALID, kCompStale);
  if (const direct_status_t rc = fetch_resident(h, mem, (size_t)h->D.G * sizeof(int32_t), label, h->comp_label, size, h->comp_size)) return rc;
  if (min_d2_built) *min_d2_built = h->rs.labels_floor();
  return DIRECT_OK;
}

direct_status_t direct_cluster_reachable_batch(direct_cluster_handle_t h, const direct_reachable_in_t* in, direct_reachable_out_t* out) {
  if (!h || !in || !out || !in->starts || !in->goals) return cfail(DIRECT_ERR_INVALID, "null argument");
  // what the arguments alone decide comes first, then what the handle holds
  if (in->n <= 0) return cfail(DIRECT_ERR_INVALID, "n must be positive");
  if (!mem_kind(in->mem_in) || !mem_kind(out->mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (in->min_d2 < 0) return cfail(DIRECT_ERR_INVALID, "min_d2 must not be negative");
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  if (!h->rs.labels_serve()) return cfail(DIRECT_ERR_INVALID, kCompStale);
  if (fc::normal_floor(in->min_d2) != h->rs.labels_floor())
    return cfail(DIRECT_ERR_INVALID, "min_d2 differs from the floor the free components were built with");
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)in->n;
  ReachDev R = {};
  R.label = h->comp_label; R.size = h->comp_size; R.n = in->n;
  R.X = h->D.max_x; R.Y = h->D.max_y; R.Z = h->D.max_z;
  hs::Stage si(in->mem_in == DIRECT_MEM_HOST), so(out->mem == DIRECT_MEM_HOST);
  hs::stage_in(si, &R.starts, in->starts, n * 3 * sizeof(int32_t));
  hs::stage_in(si, &R.goals, in->goals, n * 3 * sizeof(int32_t));
  hs::stage_out(so, &R.rtn, out->rtn, n * sizeof(int32_t));
  hs::stage_out(so, &R.goal_label, out->goal_label, n * sizeof(int32_t));
  hs::stage_out(so, &R.goal_size, out->goal_size, n * sizeof(int32_t));
  CHIP_TRY(hs::stage_upload(si, h->reach_in, h->stream));
  CHIP_TRY(hs::stage_upload(so, h->reach_out, h->stream));
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipLaunchKernelGGL(k_reach, dim3((unsigned)std::min<size_t>((n + 255) / 256, kCcBlocks)), dim3(256), 0, h->stream, R);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  e = hs::drain(h->stream, hs::stage_download(so, h->stream, e));
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("reachable_batch: ") + hipGetErrorString(e));
  return DIRECT_OK;
}

direct_status_t direct_cluster_get_known(direct_cluster_handle_t h, int32_t mem, uint8_t* known) {
  if (!h || !known) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (!h->rs.has_known()) return cfail(DIRECT_ERR_INVALID, "the handle has no known grid");
  return fetch_resident(h, mem, (size_t)h->D.G, known, h->known);
}

direct_status_t direct_cluster_set_known(direct_cluster_handle_t h, int32_t mem, const uint8_t* known) {
  if (!h) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const size_t cells = (size_t)h->D.G;
  if (!h->known) CHIP_TRY(hs::alloc_all(h->allocs, {hs::want(&h->known, cells)}));
  const uint8_t* src = known;
  if (known && mem == DIRECT_MEM_HOST) {
    CHIP_TRY(hs::grow(h->known_in, h->stream, cells));
    src = (const uint8_t*)h->known_in.p;
  }
  h->rs.known_dropped();  // the grid is about to be written: not present until the call has drained
  hipError_t e = hipSuccess;
  if (!known) {
    e = hipMemsetAsync(h->known, 0, cells, h->stream);
  } else {
    if (mem == DIRECT_MEM_HOST) e = hipMemcpyAsync(h->known_in.p, known, cells, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      const int blocks = (int)std::min<long long>(((long long)cells + 255) / 256, kScanMaxBlocks);
      hipLaunchKernelGGL(k_known_set, dim3(blocks), dim3(256), 0, h->stream, h->known, src, (long long)cells);
      e = hipGetLastError();
    }
  }
  e = hs::drain(h->stream, e);
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("set_known: ") + hipGetErrorString(e));
  h->rs.known_set();
  return DIRECT_OK;
}

direct_status_t direct_cluster_frontier(direct_cluster_handle_t h, const direct_frontier_in_t* in, const direct_frontier_out_t* out) {
  if (!h || !in || !out) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(in->mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (in->min_d2 < 0) return cfail(DIRECT_ERR_INVALID, "min_d2 must not be negative");
  if (in->min_size < 1) return cfail(DIRECT_ERR_INVALID, "min_size must be at least 1");
  if (in->capacity < 0) return cfail(DIRECT_ERR_INVALID, "capacity must not be negative");
  if (in->capacity > 0 && !out->label && !out->size && !out->centroid && !out->rep)
    return cfail(DIRECT_ERR_INVALID, "capacity without a per-component output: pass one of label, size, centroid, rep, or capacity 0");
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  if (!h->rs.has_known()) return cfail(DIRECT_ERR_INVALID, "the handle has no known grid");
  const int32_t floor = fc::normal_floor(in->min_d2);
  if (floor)
    if (const char* why = h->rs.field_refusal(floor, 0)) return cfail(DIRECT_ERR_INVALID, why);
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const Dev& D = h->D;
  const size_t G = (size_t)D.G, nb = (G + 255) / 256;
  FrontDev F = {};
  F.map = h->map; F.known = h->known; F.d2 = floor ? h->dist[0] : nullptr;
  F.X = D.max_x; F.Y = D.max_y; F.Z = D.max_z; F.G = D.G; F.nb = (int)nb;
  F.min_d2 = floor; F.min_size = in->min_size;
  F.capacity = (int)std::min<size_t>((size_t)in->capacity, G);  // no more components than voxels: the slot arrays need no more
  // the workspace of G-sized grids: words first, the mask's bytes last
  unsigned long long* lab_cnt = nullptr;
  {
    const size_t words = (4 + kFrontCounters) * sizeof(unsigned long long) + (3 * G + nb) * sizeof(int32_t);
    CHIP_TRY(hs::grow(h->front_ws, h->stream, words + G));
    char* q = (char*)h->front_ws.p;
    lab_cnt = (unsigned long long*)q; F.cnt = lab_cnt + 4; q += (4 + kFrontCounters) * sizeof(unsigned long long);
    F.label = (int32_t*)q; q += G * sizeof(int32_t);
    F.size = (int32_t*)q; q += G * sizeof(int32_t);
    F.slot = (int32_t*)q; q += G * sizeof(int32_t);
    F.wg = (int32_t*)q; q += nb * sizeof(int32_t);
    F.mask = (uint8_t*)q;
  }
  const size_t cap = (size_t)F.capacity;
  hs::Stage so(in->mem == DIRECT_MEM_HOST);
  hs::stage_scratch(so, &F.s_sum, cap * 3 * sizeof(unsigned long long));
  hs::stage_scratch(so, &F.s_key, cap * sizeof(unsigned long long));
  hs::stage_scratch(so, &F.s_label, cap * sizeof(int32_t));
  hs::stage_scratch(so, &F.s_size, cap * sizeof(int32_t));
  hs::stage_out(so, &F.o_label, out->label, cap * sizeof(int32_t), 0xff);
  hs::stage_out(so, &F.o_size, out->size, cap * sizeof(int32_t), 0xff);
  hs::stage_out(so, &F.o_centroid, out->centroid, cap * 3 * sizeof(int32_t), 0xff);
  hs::stage_out(so, &F.o_rep, out->rep, cap * 3 * sizeof(int32_t), 0xff);
  CHIP_TRY(hs::stage_upload(so, h->front_out, h->stream));
  if (h->scan_timing && !h->front_ev[0])
    for (hipEvent_t& ev : h->front_ev) CHIP_TRY(hipEventCreate(&ev));
  h->front_timed = false;
  auto tick = [&](int k) { return h->scan_timing ? hipEventRecord(h->front_ev[k], h->stream) : hipSuccess; };
  CompDev A = {};
  A.map = F.mask; A.d2 = nullptr; A.label = F.label; A.size = F.size; A.cnt = lab_cnt;
  A.X = F.X; A.Y = F.Y; A.Z = F.Z; A.G = F.G; A.min_d2 = 0;
  A.tx = gp::tiles_along(A.X); A.ty = gp::tiles_along(A.Y); A.tz = gp::tiles_along(A.Z);
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = hipMemsetAsync(lab_cnt, 0, (4 + kFrontCounters) * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(F.size, 0, G * sizeof(int32_t), h->stream);
  if (e == hipSuccess && cap) e = hipMemsetAsync(F.s_sum, 0, cap * 3 * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess && cap) e = hipMemsetAsync(F.s_key, 0xff, cap * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = tick(0);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_front_mask, dim3(F.nb), dim3(256), 0, h->stream, F);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = tick(1);
  if (e == hipSuccess) e = free_comp_launch(A, h->stream);
  if (e == hipSuccess) e = tick(2);
  if (e == hipSuccess) e = front_compact_launch(F, h->stream);
  if (e == hipSuccess) e = tick(3);
  if (e == hipSuccess) e = front_goals_launch(F, h->stream);
  if (e == hipSuccess) e = tick(4);
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  unsigned long long cnt[4 + kFrontCounters] = {};
  if (e == hipSuccess) e = hipMemcpyAsync(cnt, lab_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && out->voxel_label)
    e = hipMemcpyAsync(out->voxel_label, F.label, G * sizeof(int32_t), in->mem == DIRECT_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                       h->stream);
  e = hs::drain(h->stream, hs::stage_download(so, h->stream, e));
  if (e == hipSuccess && h->scan_timing) {
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipEventElapsedTime(&h->front_ms[k], h->front_ev[k], h->front_ev[k + 1]);
    h->front_timed = e == hipSuccess;
  }
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("frontier: ") + hipGetErrorString(e));
  if (cnt[3]) return cfail(DIRECT_ERR_DEVICE, "frontier: a union-find loop passed its trip bound (error word " + std::to_string(cnt[3]) + ")");
  if (out->stats) {
    const unsigned long long kept = cnt[4 + kFrontKept];
    out->stats[0] = (int64_t)cnt[4 + kFrontKnown]; out->stats[1] = (int64_t)cnt[4 + kFrontVoxels]; out->stats[2] = (int64_t)cnt[1];
    out->stats[3] = (int64_t)kept; out->stats[4] = (int64_t)std::min<unsigned long long>(kept, (unsigned long long)in->capacity);
    out->stats[5] = fc::stat_size(cnt[2]);
  }
  return DIRECT_OK;
}

direct_status_t direct_cluster_frontier_phase_ms(direct_cluster_handle_t h, float* ms4) {
  if (!h || !ms4) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!h->scan_timing || !h->front_timed) return cfail(DIRECT_ERR_INVALID, "no timed frontier call: set DIRECT_CLUSTER_SCAN_TIMING=1 before direct_cluster_create");
  for (int k = 0; k < 4; k++) ms4[k] = h->front_ms[k];
  return DIRECT_OK;
}

direct_status_t direct_cluster_view_gain_batch(direct_cluster_handle_t h, const direct_view_gain_in_t* in, const direct_view_gain_io_t* io) {
  if (!h || !in || !io) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!mem_kind(in->mem_in) || !mem_kind(in->mem)) return cfail(DIRECT_ERR_INVALID, kMemRefusal);
  if (in->n < 0) return cfail(DIRECT_ERR_INVALID, "n must not be negative");
  if (in->n_dirs < 1) return cfail(DIRECT_ERR_INVALID, "n_dirs must be at least 1");
  if (in->n_sets < 1) return cfail(DIRECT_ERR_INVALID, "n_sets must be at least 1");
  if (!std::isfinite(in->range_vox) || !(in->range_vox > 0.0)) return cfail(DIRECT_ERR_INVALID, "range_vox must be finite and positive");
  if (in->n > 0 && (!io->voxel || !io->dirs)) return cfail(DIRECT_ERR_INVALID, "null voxel or dirs");
  if (in->n > 0 && !io->code && !io->gain && !io->seen && !io->ends)
    return cfail(DIRECT_ERR_INVALID, "no output: pass one of code, gain, seen, ends");
  if (!vg::supported(in->range_vox))
    return cfail(DIRECT_ERR_UNSUPPORTED, "range_vox: floor(range_vox) + 2 above " + std::to_string(vg::kMaxR) + ", the box of bits would not fit in LDS");
  if (in->n_dirs > vg::kMaxDirs) return cfail(DIRECT_ERR_UNSUPPORTED, "n_dirs above " + std::to_string(vg::kMaxDirs));
  if (!h->rs.has_map()) return cfail(DIRECT_ERR_INVALID, "the handle has no map");
  if (!h->rs.has_known()) return cfail(DIRECT_ERR_INVALID, "the handle has no known grid");
  if (in->n == 0) return DIRECT_OK;
  CHIP_TRY(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)in->n;
  ViewDev V = {};
  V.S.size[0] = h->D.max_x; V.S.size[1] = h->D.max_y; V.S.size[2] = h->D.max_z;
  V.S.R = vg::box_half(in->range_vox);
  V.S.R2 = in->range_vox * in->range_vox;
  V.map = h->rs.has_open_map() ? h->open_map : h->map; V.known = h->known;  // the rays stop at what was SEEN occupied
  V.n_dirs = in->n_dirs; V.n_sets = in->n_sets; V.words = vg::box_words(V.S.R);
  hs::Stage si(in->mem_in == DIRECT_MEM_HOST), so(in->mem == DIRECT_MEM_HOST);
  hs::stage_in(si, &V.voxel, io->voxel, n * 3 * sizeof(int32_t));
  hs::stage_in(si, &V.set, io->set, n * sizeof(int32_t));
  hs::stage_in(si, &V.dirs, io->dirs, (size_t)in->n_sets * in->n_dirs * 3 * sizeof(float));
  hs::stage_scratch(so, &V.err, sizeof(unsigned int));
  hs::stage_out(so, &V.code, io->code, n * sizeof(int32_t));
  hs::stage_out(so, &V.gain, io->gain, n * sizeof(int32_t));
  hs::stage_out(so, &V.seen, io->seen, n * sizeof(int32_t));
  hs::stage_out(so, &V.ends, io->ends, n * 4 * sizeof(int32_t));
  CHIP_TRY(hs::stage_upload(si, h->view_in, h->stream));
  CHIP_TRY(hs::stage_upload(so, h->view_out, h->stream));
  const size_t lds = (size_t)V.words * sizeof(unsigned int);
  const int threads = h->view_threads ? h->view_threads : kViewThreads;
  // the largest box is past the 64 KiB a launch gets without asking; a refusal here shows as the launch's own error
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_view_gain), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)hipGetLastError();
  CHIP_TRY(hs::start(h->ev, h->stream));
  hipError_t e = hipMemsetAsync(V.err, 0, sizeof(unsigned int), h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_view_gain, dim3((unsigned)n), dim3(threads), lds, h->stream, V);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hs::stop(h->ev, h->stream);
  unsigned int err = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&err, V.err, sizeof(err), hipMemcpyDeviceToHost, h->stream);
  e = hs::drain(h->stream, hs::stage_download(so, h->stream, e));
  if (e != hipSuccess) return cfail(DIRECT_ERR_DEVICE, std::string("view_gain_batch: ") + hipGetErrorString(e));
  if (err) return cfail(DIRECT_ERR_DEVICE, "view_gain_batch: a walk left its box or passed its trip bound (error word " + std::to_string(err) + ")");
  return DIRECT_OK;
}

direct_status_t direct_cluster_set_stream(direct_cluster_handle_t h, void* hip_stream) {
  if (!h) return DIRECT_ERR_INVALID;
  h->stream = (hipStream_t)hip_stream;  // every copy, launch and event of the handle is enqueued on it from now on
  return DIRECT_OK;
}

direct_status_t direct_cluster_last_ms(direct_cluster_handle_t h, float* ms) {
  if (!h || !ms) return cfail(DIRECT_ERR_INVALID, "null argument");
  if (!h->ev.timed) return cfail(DIRECT_ERR_INVALID, "nothing has been timed yet");
  CHIP_TRY(hs::elapsed(h->ev, ms));
  return DIRECT_OK;
}

}  // extern "C"
