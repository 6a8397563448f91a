"""g++ build of direct_amd/csrc/cube_corridor_clear_math.h + cube_corridor_math.h as a program - TEST INFRASTRUCTURE of
tests/test_cube_corridor_clear_cpp.py, tests/test_gpu_cube_corridor_clear.py and tools/cube_corridor_clear_bench.py.  The program
restates direct_cluster_cube_corridor_clear_batch serially: the table in use is the map's (bytes == 1) when the floor is neutral,
else the floor table, filled entry by entry through the header's index arithmetic and summed along z, y, x as k_sat_scan does:
  table      the table in use, every entry
  corridors  a whole call: every output of the C-ABI, in either dtype, with its return codes
A second, stand-alone program drives the slot choice of the cache (floor_slot_choose).  The map, the paths and the file helpers
are those of tests/cube_corridor_harness.py."""
import os
import subprocess

import numpy as np

from tests import cube_corridor_harness as ch

ROOT = ch.ROOT

HARNESS = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cube_corridor_clear_math.h"
#include "cube_corridor_math.h"
namespace cc = direct::cubecor;
struct Map { int X, Y, Z, sz, syz; std::vector<int> sat; };
static void scan(Map& M) {  // running sums along z, then y, then x
  const int st[3] = {M.syz, M.sz, 1};
  for (int axis = 2; axis >= 0; axis--)
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
// in: int32 X, Y, Z, mode, n, cap, itr, pop_back, seg_cap, p_max, f32, min_d2; float64 res, lower[3]; uint8 map[G]; int32 d2[G]; then per mode
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[12];
  double g[4];
  if (!f || fread(h, 4, 12, f) != 12 || fread(g, 8, 4, f) != 4) return 1;
  Map M;
  M.X = h[0]; M.Y = h[1]; M.Z = h[2];
  const int mode = h[3], n = h[4], cap = h[5], itr = h[6], pop_back = h[7], S = h[8], P = h[9], f32 = h[10], min_d2 = h[11];
  const double res = g[0], *lower = g + 1;
  const size_t G = (size_t)M.X * M.Y * M.Z;
  std::vector<uint8_t> m(G);
  std::vector<int32_t> d2(G);
  rd(f, m); rd(f, d2);
  M.sz = M.Z + 1; M.syz = (M.Y + 1) * M.sz;
  M.sat.assign((size_t)(M.X + 1) * M.syz, 0);
  for (int i = 0; i < (int)M.sat.size(); i++) {
    if (cc::floor_neutral(min_d2)) {  // the map's own table: the field is not looked at
      const int v = cc::floor_entry_voxel(i, M.Y, M.Z);
      M.sat[i] = v >= 0 && m[v] == 1 ? 1 : 0;
    } else {
      M.sat[i] = cc::floor_entry(d2.data(), i, M.Y, M.Z, min_d2);
    }
  }
  scan(M);
  FILE* o = fopen(argv[2], "wb");
  if (mode == 0) {  // -> int32 table[(X+1)(Y+1)(Z+1)]
    wr(o, M.sat);
  } else {  // int32 path_xyz[n][cap][3], path_len[n] -> the outputs of the C-ABI in its order
    std::vector<int32_t> path(3 * (size_t)n * cap), len(n);
    rd(f, path); rd(f, len);
    std::vector<int32_t> n_seg(n, 0), n_planes((size_t)n * S, 0), cube_idx(6 * (size_t)n * S, 0), rtn(n, 0);
    std::vector<double> planes(4 * (size_t)n * S * P, 0.0), seeds(3 * (size_t)n * S, 0.0), ctrs(3 * (size_t)n * S, 0.0);
    std::vector<int> cube(6 * (size_t)cap), stack(cap);
    for (int b = 0; b < n; b++) {
      const int32_t* p = &path[3 * (size_t)b * cap];
      bool bad = len[b] <= 0 || len[b] > cap;
      for (int i = 0; !bad && i < len[b]; i++) {
        cube_of(M, p + 3 * i, itr, &cube[6 * i]);
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
    wr(o, n_seg); wr(o, n_planes); wr_real(o, planes, f32); wr_real(o, seeds, f32); wr_real(o, ctrs, f32); wr(o, cube_idx); wr(o, rtn);
  }
  fclose(f);
  fclose(o);
  return 0;
}
'''

# floor_slot_choose driven as a handle drives it: lines "min_d2 serial" on stdin -> "slot hit" per line
SLOTS = r'''
#include <cstdio>
#include "cube_corridor_clear_math.h"
namespace cc = direct::cubecor;
int main() {
  cc::FloorSlot s[cc::kFloorSlots] = {};
  unsigned long long clock = 0, serial;
  int min_d2;
  while (scanf("%d %llu", &min_d2, &serial) == 2) {
    int hit = -1;
    const int k = cc::floor_slot_choose(s, cc::kFloorSlots, min_d2, serial, &hit);
    if (k < 0 || k >= cc::kFloorSlots) return 1;
    if (!hit) { s[k].min_d2 = min_d2; s[k].serial = serial; s[k].valid = 1; }
    s[k].used = ++clock;
    printf("%d %d\n", k, hit);
  }
  return 0;
}
'''

CXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "direct_amd", "csrc")]


def build(workdir):
    src = os.path.join(str(workdir), "cube_corridor_clear_harness.cpp")
    exe = os.path.join(str(workdir), "cube_corridor_clear_harness")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(CXX + [src, "-o", exe])
    return str(workdir), exe


def build_slots(workdir, extra=()):
    src = os.path.join(str(workdir), "floor_slots.cpp")
    exe = os.path.join(str(workdir), "floor_slots")
    with open(src, "w") as f:
        f.write(SLOTS)
    subprocess.check_call(CXX + list(extra) + [src, "-o", exe])
    return exe


def slot_choices(exe, calls):
    """calls: [(min_d2, serial)] in order -> [(slot, hit)]"""
    out = subprocess.run([exe], input="".join("%d %d\n" % c for c in calls), capture_output=True, text=True, check=True).stdout.split()
    return [(int(out[i]), int(out[i + 1])) for i in range(0, len(out), 2)]


def brute_d2(grid):
    """the exact squared distance of every voxel to the nearest occupied one, by NumPy brute force (uncapped; the map is not empty)"""
    occ = np.argwhere(np.asarray(grid) == 1).astype(np.int64)
    idx = np.indices(grid.shape).reshape(3, -1).T.astype(np.int64)
    best = np.full(len(idx), np.iinfo(np.int64).max)
    for o in occ:
        best = np.minimum(best, ((idx - o) ** 2).sum(1))
    return best.reshape(grid.shape).astype(np.int32)


def thresholded(d2, min_d2):
    """the map on which the PLAIN call gives the clear call's result"""
    return (np.asarray(d2) < min_d2).astype(np.uint8)


def _call(harness, grid, d2, min_d2, mode, n, arrays, cap=0, itr=1000, pop_back=1, seg_cap=0, p_max=6, f32=0, res=ch.RES, lower=ch.LOWER):
    d, exe = harness
    grid = np.ascontiguousarray(grid, np.uint8)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        np.array(list(grid.shape) + [mode, n, cap, itr, int(pop_back), seg_cap, p_max, int(f32), int(min_d2)], np.int32).tofile(f)
        np.array([res] + list(lower), np.float64).tofile(f)
        grid.tofile(f)
        np.ascontiguousarray(d2, np.int32).reshape(grid.shape).tofile(f)
        for a in arrays:
            np.ascontiguousarray(a, np.int32).tofile(f)
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    os.remove(fout)
    return raw


def table(harness, grid, d2, min_d2):
    """-> the table in use [(X+1)][(Y+1)][(Z+1)]"""
    raw = _call(harness, grid, d2, min_d2, 0, 0, [])
    shape = tuple(s + 1 for s in np.asarray(grid).shape)
    t, off = ch._take(raw, 0, np.int32, shape)
    assert off == len(raw)
    return t


def corridors(harness, grid, d2, min_d2, paths, path_len, res=ch.RES, lower=ch.LOWER, itr=1000, pop_back=True, seg_capacity=40, p_max=6,
              dtype=np.float64):
    """the outputs of ClusterGenerator.cube_corridors_clear for the same arguments (without info)"""
    paths = np.ascontiguousarray(paths, np.int32)
    path_len = np.ascontiguousarray(path_len, np.int32)
    B, cap = paths.shape[0], paths.shape[1]
    S, P, real = int(seg_capacity), int(p_max), np.dtype(dtype)
    raw = _call(harness, grid, d2, min_d2, 2, B, [paths, path_len], cap=cap, itr=itr, pop_back=pop_back, seg_cap=S, p_max=P,
                f32=real == np.float32, res=res, lower=lower)
    out, off = {}, 0
    for k, dt, shape in (("n_seg", np.int32, (B,)), ("n_planes", np.int32, (B, S)), ("planes", real, (B, S, P, 4)), ("seeds", real, (B, S, 3)),
                         ("centers", real, (B, S, 3)), ("cube_idx", np.int32, (B, S, 6)), ("rtn", np.int32, (B,))):
        out[k], off = ch._take(raw, off, dt, shape)
    assert off == len(raw)
    return out


def rows40():
    """the 40 rows of tests/test_gpu_cube_corridor.py::rows: the named cases inside the map, then random walks (seed 9)"""
    paths = []
    for c in ch.named_cases():
        if c["name"] != "outside_voxel":
            paths += [p for p in c["paths"]]
    paths += ch.random_paths(ch.crafted_map(), 40 - len(paths), seed=9)
    assert len(paths) == 40
    return [np.asarray(p, np.int32) for p in paths]


def guarantee(cube_idx, n_seg, seeds_vox, d2, min_d2):
    """the integer guarantee: every voxel of every kept cube other than its seed voxel has d2 >= min_d2.  seeds_vox [B][S][3] are
    the seed voxels.  -> (cubes checked, cubes larger than one voxel)"""
    checked = large = 0
    for b in range(len(n_seg)):
        for k in range(min(int(n_seg[b]), cube_idx.shape[1])):
            c, s = cube_idx[b, k], seeds_vox[b, k]
            blk = d2[c[0]:c[3] + 1, c[1]:c[4] + 1, c[2]:c[5] + 1].copy()
            assert (c[:3] <= s).all() and (s <= c[3:]).all(), (b, k)
            blk[tuple(s - c[:3])] = np.iinfo(np.int32).max
            assert blk.min() >= min_d2, (b, k, c.tolist(), int(blk.min()))
            checked += 1
            large += blk.size > 1
    return checked, large
