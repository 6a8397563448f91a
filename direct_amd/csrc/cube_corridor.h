// Kernels of direct_cluster_cube_corridor_batch (include/direct_cluster.h, "cube corridors"): the corridors of a batch of grid
// paths in the reference's is_cluster_on == false mode, in which a polytope is the inflated cube of its seed voxel - a pure
// function of the voxel and the map.  Included from direct_cluster.hip inside its anonymous namespace, after Dev and
// box_obstacles; the arithmetic is cube_corridor_math.h (plain C++, also compiled by g++ for tests/cube_corridor_harness.py).
//
//   k_cube_inflate  the cube of EVERY path point of every row, one lane per (row, point) slot: sum(path_len) independent chains
//                   of table queries in flight instead of one chain per row as long as its whole corridor
//   k_cube_walk     one wave per row: the walk selects the cubes that form the corridor (a stack of path indices), then the
//                   wave's lanes write the row's outputs, one polytope per lane, zeros behind them
// No kernel waits for another workgroup, there are no atomics, and every loop is bounded by the data's sizes: each kernel ends
// on its own.  A slot's cube and a row's corridor depend on nothing but that slot / row, so no output depends on the launch shape.
#pragma once

namespace cc = ::direct::cubecor;

struct CubeDev {
  int batch, path_cap, seg_cap, p_max, itr_inflate_max, pop_back;
  double res, lower[3];
  const int32_t* path_xyz;  // [batch][path_cap][3]
  const int32_t* path_len;  // [batch]
  int* cube;                // [batch][path_cap][6] workspace: lo xyz, hi xyz; cube[0] == cc::kNoCube: no cube
  int* stack;               // [batch][path_cap] workspace: path index of every polytope of the row's corridor
  int32_t *n_seg, *n_planes, *cube_idx, *rtn;  // outputs, any may be null
  void *planes, *seeds, *centers;              // in the call's plane_dtype
};

// One lane per slot, striding over the slots.  A query is eight independent loads (box_obstacles) and the chain from one query
// to the next is serial, so a lane is latency-bound; the lanes of a wave hold neighbouring points of one path, whose cubes are
// alike, and run about equally long.
__global__ __launch_bounds__(64) void k_cube_inflate(Dev D, CubeDev A) {
  const size_t slots = (size_t)A.batch * A.path_cap;
  for (size_t s = (size_t)blockIdx.x * 64 + threadIdx.x; s < slots; s += (size_t)gridDim.x * 64) {
    const int row = (int)(s / A.path_cap), i = (int)(s - (size_t)row * A.path_cap);
    const int len = A.path_len[row];
    int c[6] = {cc::kNoCube, 0, 0, 0, 0, 0};
    if (i < len && len <= A.path_cap) {
      const int x = A.path_xyz[3 * s], y = A.path_xyz[3 * s + 1], z = A.path_xyz[3 * s + 2];
      if (x >= 0 && x < D.max_x && y >= 0 && y < D.max_y && z >= 0 && z < D.max_z)
        cc::inflate([&](int x0, int y0, int z0, int x1, int y1, int z1) { return box_obstacles(D, x0, y0, z0, x1, y1, z1); }, D.max_x,
                    D.max_y, D.max_z, x, y, z, A.itr_inflate_max, c);
    }
    for (int k = 0; k < 6; k++) A.cube[6 * s + k] = c[k];
  }
}

template <typename Real>
__device__ __forceinline__ void cube_store(void* base, size_t at, double v) {
  if (base) ((Real*)base)[at] = (Real)v;  // float: one rounding of the double
}

// One wave per row.  Lanes 0 .. 5 hold the planes of the latest polytope, lanes 6 .. 11 those of the last but one; the outside
// test of a point is one ballot.  The corridor is kept as a stack of path indices (every lane stores the same value, so each
// lane later reads what it wrote itself); a polytope's planes are recomputed from its cube whenever the stack changes.
template <typename Real>
__global__ __launch_bounds__(64) void k_cube_walk(CubeDev A) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int len = A.path_len[row];
  const int32_t* path = A.path_xyz + (size_t)row * A.path_cap * 3;
  const int* cube = A.cube + (size_t)row * A.path_cap * 6;
  int* stack = A.stack + (size_t)row * A.path_cap;
  bool bad = len <= 0 || len > A.path_cap;
  if (!bad) {
    int none = 0;
    for (int i = lane; i < len; i += 64) none |= cube[6 * i] == cc::kNoCube;
    bad = __any(none) != 0;
  }
  int n = 0;
  if (!bad) {
    double mine[4] = {0.0, 0.0, 0.0, 0.0};
    int s_latest = -1, s_prev = -1;
    auto reload = [&]() {
      const int s = lane < 6 ? s_latest : (lane < 12 ? s_prev : -1);
      if (s < 0) return;
      double pl[4 * cc::kPlanes], ctr[3];
      cc::cube_polytope(cube + 6 * s, A.res, A.lower, pl, ctr);
      const int t = lane < 6 ? lane : lane - 6;
#pragma unroll
      for (int k = 0; k < cc::kPlanes; k++)
        if (k == t)
          for (int q = 0; q < 4; q++) mine[q] = pl[4 * k + q];
    };
    double lst[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int i = 0; i < len; i++) {
      double cur[3];
      cc::index2coord(path + 3 * i, A.res, A.lower, cur);
      if (cur[0] == lst[0] && cur[1] == lst[1] && cur[2] == lst[2]) continue;
      unsigned long long m = __ballot(lane < 12 && cc::plane_excludes(cur, mine));
      if (A.pop_back && n > 1 && !(m & 0xfc0ull)) {  // inside the last but one: the last one goes
        n--;
        s_latest = s_prev;
        s_prev = n > 1 ? stack[n - 2] : -1;
        reload();
        m = __ballot(lane < 12 && cc::plane_excludes(cur, mine));
      }
      if (n == 0 || (m & 0x3full)) {
        stack[n++] = i;
        s_prev = s_latest;
        s_latest = i;
        reload();
      }
      for (int a = 0; a < 3; a++) lst[a] = cur[a];
    }
  }
  // the row's outputs: polytope k of the corridor by lane k % 64, zeros from the corridor's end to seg_cap
  const int nv = n < A.seg_cap ? n : A.seg_cap;
  for (int k = lane; k < A.seg_cap; k += 64) {
    const size_t o = (size_t)row * A.seg_cap + k;
    double pl[4 * cc::kPlanes] = {0.0}, ctr[3] = {0.0, 0.0, 0.0}, seed[3] = {0.0, 0.0, 0.0};
    int c[6] = {0, 0, 0, 0, 0, 0};
    if (k < nv) {
      const int s = stack[k];
      for (int q = 0; q < 6; q++) c[q] = cube[6 * s + q];
      cc::cube_polytope(c, A.res, A.lower, pl, ctr);
      cc::index2coord(path + 3 * s, A.res, A.lower, seed);
    }
    if (A.n_planes) A.n_planes[o] = k < nv ? cc::kPlanes : 0;
    if (A.cube_idx)
      for (int q = 0; q < 6; q++) A.cube_idx[6 * o + q] = c[q];
#pragma unroll
    for (int q = 0; q < 4 * cc::kPlanes; q++) cube_store<Real>(A.planes, o * 4 * A.p_max + q, pl[q]);
    for (int q = 4 * cc::kPlanes; q < 4 * A.p_max; q++) cube_store<Real>(A.planes, o * 4 * A.p_max + q, 0.0);  // the stride is the caller's
    for (int a = 0; a < 3; a++) {
      cube_store<Real>(A.seeds, 3 * o + a, seed[a]);
      cube_store<Real>(A.centers, 3 * o + a, ctr[a]);
    }
  }
  if (lane == 0) {
    if (A.n_seg) A.n_seg[row] = n;
    if (A.rtn) A.rtn[row] = bad ? DIRECT_CUBE_CORRIDOR_BAD_PATH : (n > A.seg_cap ? DIRECT_CUBE_CORRIDOR_OVERFLOW : DIRECT_CUBE_CORRIDOR_OK);
  }
}
