"""g++ build of direct_amd/csrc/cube_corridor_math.h and cube_corridor_clear_math.h as ONE program - TEST INFRASTRUCTURE of
tests/test_cube_corridor_cpp.py, tests/test_cube_corridor_restatement.py, tests/test_gpu_cube_corridor.py,
tools/cube_corridor_bench.py and, through tests/cube_corridor_clear_harness.py, of the radius-aware call's tests.  The program
restates direct_cluster_cube_corridor_batch and direct_cluster_cube_corridor_clear_batch serially on a summed-area table (the
library's layout) that one header word has filled in one of two ways, each the witness of the other:
  map    inclusion-exclusion over the map's bytes == 1
  floor  entry by entry through the clear header's index arithmetic - the map's own table when the floor is neutral, else the
         floor table of the distance field -, then running sums along z, y, x as k_sat_scan takes them
and runs the headers' functions:
  cubes      the cube of a list of seed voxels, with the number of table queries each took
  polytopes  planes, centre and degenerate flag of a list of cubes
  table      the table in use, every entry
  corridors  a whole call: every output of the C-ABI, in either dtype, with its return codes, then the queries per path voxel
This file also holds the map and the named paths that the CPU and the GPU tests share."""
import numpy as np

from tests import cpp_program as cpp

ROOT = cpp.ROOT
OK, OVERFLOW, BAD_PATH = 0, 1, 2
NO_CUBE = -1
RES, LOWER = 0.2, np.array([-2.4, -2.0, 0.0])
DIMS = (24, 20, 12)
CUBES, POLYTOPES, TABLE, CORRIDORS = 0, 1, 2, 3   # the program's modes
FROM_MAP, FROM_FLOOR = 0, 1                       # and its two ways to fill the table

HARNESS = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "cube_corridor_clear_math.h"
#include "cube_corridor_math.h"
namespace cc = direct::cubecor;
struct Map { int X, Y, Z, sz, syz; std::vector<uint8_t> m; std::vector<int32_t> d2; std::vector<int> sat; };
static void fill_from_map(Map& M) {
  for (int x = 1; x <= M.X; x++)
    for (int y = 1; y <= M.Y; y++)
      for (int z = 1; z <= M.Z; z++) {
        auto S = [&](int a, int b, int c) { return M.sat[a * M.syz + b * M.sz + c]; };
        M.sat[x * M.syz + y * M.sz + z] = (M.m[((x - 1) * M.Y + (y - 1)) * M.Z + (z - 1)] == 1 ? 1 : 0) + S(x - 1, y, z) + S(x, y - 1, z) + S(x, y, z - 1) -
                                          S(x - 1, y - 1, z) - S(x - 1, y, z - 1) - S(x, y - 1, z - 1) + S(x - 1, y - 1, z - 1);
      }
}
static void fill_from_floor(Map& M, int min_d2) {
  for (int i = 0; i < (int)M.sat.size(); i++) {
    if (cc::floor_neutral(min_d2)) {  // the map's own table: the field is not looked at
      const int v = cc::floor_entry_voxel(i, M.Y, M.Z);
      M.sat[i] = v >= 0 && M.m[v] == 1 ? 1 : 0;
    } else {
      M.sat[i] = cc::floor_entry(M.d2.data(), i, M.Y, M.Z, min_d2);
    }
  }
  const int st[3] = {M.syz, M.sz, 1};
  for (int axis = 2; axis >= 0; axis--)  // running sums along z, then y, then x
    for (size_t i = 0; i < M.sat.size(); i++) {
      const int c[3] = {(int)(i / M.syz), (int)(i % M.syz) / M.sz, (int)(i % M.sz)};
      if (c[axis] > 0) M.sat[i] += M.sat[i - st[axis]];
    }
}
static int box(const Map& M, int x0, int y0, int z0, int x1, int y1, int z1) {
  auto S = [&](int a, int b, int c) { return M.sat[a * M.syz + b * M.sz + c]; };
  return S(x1 + 1, y1 + 1, z1 + 1) - S(x0, y1 + 1, z1 + 1) - S(x1 + 1, y0, z1 + 1) - S(x1 + 1, y1 + 1, z0) + S(x0, y0, z1 + 1) + S(x0, y1 + 1, z0) +
         S(x1 + 1, y0, z0) - S(x0, y0, z0);
}
static int cube_of(const Map& M, const int32_t* s, int itr, int* c) {
  c[0] = cc::kNoCube; c[1] = c[2] = c[3] = c[4] = c[5] = 0;
  if (s[0] < 0 || s[0] >= M.X || s[1] < 0 || s[1] >= M.Y || s[2] < 0 || s[2] >= M.Z) return 0;
  return cc::inflate([&](int x0, int y0, int z0, int x1, int y1, int z1) { return box(M, x0, y0, z0, x1, y1, z1); }, M.X, M.Y, M.Z, s[0], s[1],
                     s[2], itr, c);
}
template <typename T> static void rd(FILE* f, std::vector<T>& v) { if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(1); }
template <typename T> static void wr(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }
static void wr_real(FILE* f, const std::vector<double>& v, int f32) {
  if (!f32) { wr(f, v); return; }
  std::vector<float> w(v.size());
  for (size_t i = 0; i < v.size(); i++) w[i] = (float)v[i];
  wr(f, w);
}
// in: int32 X, Y, Z, mode, n, cap, itr, pop_back, seg_cap, p_max, f32, min_d2, fill; float64 res, lower[3]; uint8 map[G];
// with fill == 1 int32 d2[G]; then per mode (below)
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[13];
  double g[4];
  if (!f || fread(h, 4, 13, f) != 13 || fread(g, 8, 4, f) != 4) return 1;
  Map M;
  M.X = h[0]; M.Y = h[1]; M.Z = h[2];
  const int mode = h[3], n = h[4], cap = h[5], itr = h[6], pop_back = h[7], S = h[8], P = h[9], f32 = h[10], min_d2 = h[11], fill = h[12];
  const double res = g[0], *lower = g + 1;
  M.m.resize((size_t)M.X * M.Y * M.Z);
  rd(f, M.m);
  M.sz = M.Z + 1; M.syz = (M.Y + 1) * M.sz;
  M.sat.assign((size_t)(M.X + 1) * M.syz, 0);
  if (fill == 1) {
    M.d2.resize(M.m.size());
    rd(f, M.d2);
    fill_from_floor(M, min_d2);
  } else {
    fill_from_map(M);
  }
  FILE* o = fopen(argv[2], "wb");
  if (mode == 2) {  // -> int32 table[(X+1)(Y+1)(Z+1)]
    wr(o, M.sat);
  } else if (mode == 0) {  // int32 seeds[n][3] -> int32 cube[n][6], queries[n]
    std::vector<int32_t> seeds(3 * (size_t)n), cube(6 * (size_t)n), q(n);
    rd(f, seeds);
    for (int i = 0; i < n; i++) q[i] = cube_of(M, &seeds[3 * i], itr, &cube[6 * i]);
    wr(o, cube); wr(o, q);
  } else if (mode == 1) {  // int32 cube[n][6] -> float64 planes[n][6][4], center[n][3]; int32 degenerate[n]
    std::vector<int32_t> cube(6 * (size_t)n), deg(n);
    std::vector<double> planes(24 * (size_t)n), ctr(3 * (size_t)n);
    rd(f, cube);
    for (int i = 0; i < n; i++) deg[i] = cc::cube_polytope(&cube[6 * i], res, lower, &planes[24 * i], &ctr[3 * i]);
    wr(o, planes); wr(o, ctr); wr(o, deg);
  } else {  // int32 path_xyz[n][cap][3], path_len[n] -> the outputs of the C-ABI in its order, then int32 queries[n][cap]
    std::vector<int32_t> path(3 * (size_t)n * cap), len(n);
    rd(f, path); rd(f, len);
    std::vector<int32_t> n_seg(n, 0), n_planes((size_t)n * S, 0), cube_idx(6 * (size_t)n * S, 0), rtn(n, 0), queries((size_t)n * cap, 0);
    std::vector<double> planes(4 * (size_t)n * S * P, 0.0), seeds(3 * (size_t)n * S, 0.0), ctrs(3 * (size_t)n * S, 0.0);
    std::vector<int> cube(6 * (size_t)cap), stack(cap);
    for (int b = 0; b < n; b++) {
      const int32_t* p = &path[3 * (size_t)b * cap];
      bool bad = len[b] <= 0 || len[b] > cap;
      for (int i = 0; !bad && i < len[b]; i++) {
        queries[(size_t)b * cap + i] = cube_of(M, p + 3 * i, itr, &cube[6 * i]);
        bad = cube[6 * i] == cc::kNoCube;
      }
      if (bad) { rtn[b] = 2; continue; }
      const int ns = cc::walk(p, len[b], cube.data(), res, lower, pop_back, stack.data());
      n_seg[b] = ns;
      rtn[b] = ns > S ? 1 : 0;
      for (int k = 0; k < ns && k < S; k++) {
        const size_t at = (size_t)b * S + k;
        const int s = stack[k];
        n_planes[at] = cc::kPlanes;
        for (int q = 0; q < 6; q++) cube_idx[6 * at + q] = cube[6 * s + q];
        cc::cube_polytope(&cube[6 * s], res, lower, &planes[4 * at * P], &ctrs[3 * at]);
        cc::index2coord(p + 3 * s, res, lower, &seeds[3 * at]);
      }
    }
    wr(o, n_seg); wr(o, n_planes); wr_real(o, planes, f32); wr_real(o, seeds, f32); wr_real(o, ctrs, f32); wr(o, cube_idx); wr(o, rtn); wr(o, queries);
  }
  fclose(f);
  fclose(o);
  return 0;
}
'''


def build(workdir):
    return str(workdir), cpp.compile_program(workdir, "cube_corridor_harness", HARNESS, ["-Wno-unknown-pragmas"])


def _call(harness, grid, mode, n, arrays, layout, cap=0, itr=1000, pop_back=1, seg_cap=0, p_max=6, f32=0, res=RES, lower=LOWER, floor=None):
    """floor: None - the table from the map's bytes -, or (d2, min_d2) - the table through the clear header"""
    grid = np.ascontiguousarray(grid, np.uint8)
    field, min_d2 = ([], 0) if floor is None else ([np.ascontiguousarray(floor[0], np.int32).reshape(grid.shape)], int(floor[1]))
    fill = FROM_MAP if floor is None else FROM_FLOOR
    raw = cpp.exchange(harness, list(grid.shape) + [mode, n, cap, itr, int(pop_back), seg_cap, p_max, int(f32), min_d2, fill],
                       [res] + list(lower), [grid] + field + arrays)
    return cpp.unpack(raw, layout)


def cubes(harness, grid, seeds, itr=1000):
    """-> (cube [n][6] lo xyz, hi xyz; queries [n])"""
    seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1, 3)
    n = len(seeds)
    r = _call(harness, grid, CUBES, n, [seeds], (("cube", np.int32, (n, 6)), ("queries", np.int32, (n,))), itr=itr)
    return r["cube"], r["queries"]


def polytopes(harness, cube, res=RES, lower=LOWER):
    """-> (planes [n][6][4], center [n][3], degenerate [n])"""
    cube = np.ascontiguousarray(cube, np.int32).reshape(-1, 6)
    n = len(cube)
    r = _call(harness, np.zeros((1, 1, 1), np.uint8), POLYTOPES, n, [cube],
              (("planes", np.float64, (n, 6, 4)), ("center", np.float64, (n, 3)), ("degenerate", np.int32, (n,))), res=res, lower=lower)
    return r["planes"], r["center"], r["degenerate"]


def table(harness, grid, floor=None):
    """-> the table in use [(X+1)][(Y+1)][(Z+1)]"""
    return _call(harness, grid, TABLE, 0, [], (("table", np.int32, tuple(s + 1 for s in np.asarray(grid).shape)),), floor=floor)["table"]


def corridors(harness, grid, paths, path_len, res=RES, lower=LOWER, itr=1000, pop_back=True, seg_capacity=32, p_max=6, dtype=np.float64,
              floor=None):
    """the outputs of ClusterGenerator.cube_corridors - with floor = (d2, min_d2) of cube_corridors_clear, without info - for the
    same arguments, plus queries [B][path_capacity]"""
    paths = np.ascontiguousarray(paths, np.int32)
    path_len = np.ascontiguousarray(path_len, np.int32)
    B, cap = paths.shape[0], paths.shape[1]
    S, P, real = int(seg_capacity), int(p_max), np.dtype(dtype)
    layout = (("n_seg", np.int32, (B,)), ("n_planes", np.int32, (B, S)), ("planes", real, (B, S, P, 4)), ("seeds", real, (B, S, 3)),
              ("centers", real, (B, S, 3)), ("cube_idx", np.int32, (B, S, 6)), ("rtn", np.int32, (B,)), ("queries", np.int32, (B, cap)))
    return _call(harness, grid, CORRIDORS, B, [paths, path_len], layout, cap=cap, itr=itr, pop_back=pop_back, seg_cap=S, p_max=P,
                 f32=real == np.float32, res=res, lower=lower, floor=floor)


# ---- the map and the paths the CPU and the GPU tests share ----------------------------------------------------------------

def pack_paths(paths, cap=40):
    """list of [n][3] -> (path_xyz [B][cap][3], path_len [B]); a path longer than cap keeps its length (a BAD_PATH row)"""
    xyz = np.zeros((len(paths), cap, 3), np.int32)
    n = np.zeros(len(paths), np.int32)
    for b, p in enumerate(paths):
        p = np.asarray(p, np.int32).reshape(-1, 3)
        xyz[b, :min(len(p), cap)] = p[:cap]
        n[b] = len(p)
    return xyz, n


def line(a, b):
    """the voxels from a to b, both included, one axis after the other (x, then y, then z)"""
    cur, out = list(a), [list(a)]
    for ax in range(3):
        while cur[ax] != b[ax]:
            cur[ax] += 1 if b[ax] > cur[ax] else -1
            out.append(list(cur))
    return out


def random_map(seed, density):
    return (np.random.default_rng(seed).random(DIMS) < density).astype(np.uint8)


def crafted_map():
    """24 x 20 x 12, free but for: a closed room with one door (x 2..8, y 2..8, z 2..8; free inside 3..7; door at (8, 5, 5)); a free
    voxel whose six face neighbours are occupied (13, 4, 4); a tunnel one voxel wide along x (x 11..20 at y = 12, z = 5, walls around it,
    open at x = 21); a lone occupied voxel in open space (17, 17, 9); and a post at (6, 15, 0..11) that the round order meets
    differently from axis-by-axis growth."""
    g = np.zeros(DIMS, np.uint8)
    g[2:9, 2:9, 2:9] = 1
    g[3:8, 3:8, 3:8] = 0
    g[8, 5, 5] = 0
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        g[13 + d[0], 4 + d[1], 4 + d[2]] = 1
    g[10:21, 11:14, 4:7] = 1
    g[11:21, 12, 5] = 0
    g[17, 17, 9] = 1
    g[6, 15, :] = 1
    return g


def named_cases():
    """-> list of dict(name, paths (list of [n][3]), res, pop_back, seg_capacity, rtn or None): every case a path of at most 40 voxels
    on crafted_map().  The tests assert for each that what its name says really happens."""
    room = line([4, 4, 4], [6, 6, 6])
    uturn = line([5, 5, 5], [10, 5, 5]) + line([10, 6, 5], [10, 9, 5]) + line([10, 8, 5], [10, 5, 5]) + line([9, 5, 5], [5, 5, 5])
    c = [
        dict(name="obstacle_faces", paths=[room]),
        dict(name="border_faces", paths=[line([1, 18, 10], [22, 18, 10]), line([22, 1, 1], [22, 10, 1])]),
        dict(name="round_order", paths=[[[4, 12, 6]]]),
        dict(name="enclosed_seed", paths=[[[13, 4, 4]]]),
        dict(name="thin_corridor", paths=[line([12, 12, 5], [22, 12, 5])]),
        dict(name="occupied_seed", paths=[[[17, 17, 9], [17, 17, 10]]]),
        dict(name="repeated_points", paths=[[[4, 4, 4]] * 3 + line([4, 4, 4], [9, 5, 5])[1:] + [[9, 5, 5]] * 2 + [[10, 5, 5]]]),
        dict(name="single_voxel_path", paths=[[[20, 3, 3]]]),
        dict(name="u_turn", paths=[uturn], pop_back=True),
        dict(name="u_turn_no_pop", paths=[uturn], pop_back=False),
        dict(name="resolution_0.01", paths=[line([5, 5, 5], [11, 5, 5]), line([12, 12, 5], [22, 14, 5])], res=0.01),
        dict(name="seg_capacity_short", paths=[uturn, room], pop_back=False, seg_capacity="one_short", rtn=[OVERFLOW, OK]),
        dict(name="outside_voxel", paths=[line([20, 17, 3], [23, 17, 3]) + [[24, 17, 3]], room, [[0, -1, 0]], [[0, 0, 12]]],
             rtn=[BAD_PATH, OK, BAD_PATH, BAD_PATH]),
    ]
    for k in c:
        k.setdefault("res", RES)
        k.setdefault("pop_back", True)
        k.setdefault("seg_capacity", 32)
        k.setdefault("rtn", None)
        assert all(len(p) <= 40 for p in k["paths"])
    return c


def random_paths(grid, n, seed, length=40):
    """n random walks of `length` voxels on the map, steps to any of the 26 neighbours inside the map, occupied voxels included"""
    rng = np.random.default_rng(seed)
    dims = np.array(grid.shape)
    out = []
    for _ in range(n):
        p = [rng.integers(0, dims)]
        heading = rng.integers(-1, 2, 3)
        while len(p) < length:
            if rng.random() < 0.3:
                heading = rng.integers(-1, 2, 3)
            p.append(np.clip(p[-1] + heading, 0, dims - 1))
        out.append(np.array(p, np.int32))
    return out
