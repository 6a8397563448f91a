"""Free-space components and reachability (include/direct_cluster.h, "free-space components") - TEST INFRASTRUCTURE of
tests/test_free_comp_restatement.py, tests/test_free_comp_cpp.py and tests/test_gpu_free_comp.py.  Two sides:
  restate / witness_codes   an independent NumPy restatement: the enterable voxels from the map and a brute-force D2
                            (tests/dist_field_harness.py), a stack flood fill over the 26 neighbours, label = smallest index, sizes
                            by counting; and for pairs a flood fill from the start's neighbours (no labels involved).
  build / run               direct_amd/csrc/free_comp_math.h compiled by g++ into one stand-alone program that emulates the tile
                            pass, the merge pass and the flatten as lane loops with plain reads and writes, and the pair rule.
and the maps and pairs the CPU and GPU tests share."""
import os
import subprocess

import numpy as np

from tests import dist_field_harness as dh
from tests.cpp_program import compile_program

ROOT = dh.ROOT
OK, NO_PATH, BAD_ENDPOINT = 0, 1, 2
DIMS = (24, 20, 12)      # tiles 3 x 3 x 2, partial in y and z
DIMS_BIG = (40, 36, 20)
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


# ---- the NumPy restatement ----------------------------------------------------------------------------------------------
def enterable(grid, d2=None, min_d2=0):
    grid = np.asarray(grid)
    return (grid == 0) if min_d2 <= 1 else ((grid == 0) & (np.asarray(d2) >= min_d2))


def restate(grid, d2=None, min_d2=0):
    """-> (label, size, stats[4]) by a stack flood fill in ascending index order: the first voxel of a component met is its
    smallest index"""
    ent = enterable(grid, d2, min_d2)
    X, Y, Z = ent.shape
    pad = np.zeros((X + 2, Y + 2, Z + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = ent
    free = pad.ravel().tolist()
    PY, PZ = Y + 2, Z + 2
    step = [dx * PY * PZ + dy * PZ + dz for dx, dy, dz in OFFSETS]
    label = np.full(ent.shape, -1, np.int32)
    size = np.zeros(ent.shape, np.int32)
    lab = label.reshape(-1)
    for idx in np.flatnonzero(ent.ravel()):
        if lab[idx] >= 0:
            continue
        x, r = divmod(int(idx), Y * Z)
        y, z = divmod(r, Z)
        p0 = (x + 1) * PY * PZ + (y + 1) * PZ + (z + 1)
        free[p0] = False
        stack, members = [p0], []
        while stack:
            p = stack.pop()
            members.append(p)
            for s in step:
                q = p + s
                if free[q]:
                    free[q] = False
                    stack.append(q)
        m = np.array(members)
        px, r = np.divmod(m, PY * PZ)
        py, pz = np.divmod(r, PZ)
        lin = ((px - 1) * Y + (py - 1)) * Z + (pz - 1)
        assert lin.min() == idx
        lab[lin] = idx
        size.reshape(-1)[lin] = len(lin)
    return label, size, stats_of(label, size)


def stats_of(label, size):
    lab, siz = label.reshape(-1), size.reshape(-1)
    roots = np.flatnonzero(lab == np.arange(lab.size))
    if len(roots) == 0:
        return np.array([0, 0, 0, -1], np.int64)
    big = siz[roots].max()
    return np.array([(lab >= 0).sum(), len(roots), big, roots[siz[roots] == big].min()], np.int64)


def flood(ent, seeds):
    """the enterable voxels reachable from `seeds` (a bool array; seeds that are not enterable do not count), by dilation"""
    reach = seeds & ent
    while True:
        pad = np.pad(reach, 1)
        grown = np.zeros_like(reach)
        for dx in (0, 1, 2):
            for dy in (0, 1, 2):
                for dz in (0, 1, 2):
                    grown |= pad[dx:dx + reach.shape[0], dy:dy + reach.shape[1], dz:dz + reach.shape[2]]
        grown &= ent
        if (grown == reach).all():
            return reach
        reach = grown


def witness_codes(grid, starts, goals, d2=None, min_d2=0):
    """the code of every pair WITHOUT labels: a flood fill from the start's 26 neighbours over enterable voxels (what the path
    calls' relaxation can reach: the start's own byte is never looked at)"""
    ent = enterable(grid, d2, min_d2)
    dims = np.array(ent.shape)
    out = np.zeros(len(starts), np.int32)
    cache = {}
    for i, (s, g) in enumerate(zip(np.asarray(starts), np.asarray(goals))):
        if ((s < 0) | (s >= dims) | (g < 0) | (g >= dims)).any():
            out[i] = BAD_ENDPOINT
        elif (s == g).all():
            out[i] = OK
        else:
            key = tuple(int(v) for v in s)
            if key not in cache:
                seeds = np.zeros(ent.shape, bool)
                for o in OFFSETS:
                    n = s + np.array(o)
                    if ((n >= 0) & (n < dims)).all():
                        seeds[tuple(n)] = True
                cache[key] = flood(ent, seeds)
            out[i] = OK if cache[key][tuple(g)] else NO_PATH
    return out


# ---- maps ---------------------------------------------------------------------------------------------------------------
def serpentine(dims=DIMS):
    """one free voxel-wide line through every tile: along x in rows (y, z) on a lattice of step 2, joined at alternating ends"""
    g = np.ones(dims, np.uint8)
    rows = [(y, z) for z in range(0, dims[2], 2) for y in (range(0, dims[1], 2) if (z // 2) % 2 == 0 else range(dims[1] - 2 + dims[1] % 2, -1, -2))]
    for i, (y, z) in enumerate(rows):
        g[:, y, z] = 0
        if i + 1 < len(rows):
            y2, z2 = rows[i + 1]
            x = dims[0] - 1 if i % 2 == 0 else 0
            g[x, min(y, y2):max(y, y2) + 1, min(z, z2):max(z, z2) + 1] = 0
    return g


def far_end(dims=DIMS):
    """a component whose smallest-index voxel (x = 0) is joined to the rest only through the far end (x = X - 1): two parallel
    lines along x, joined at x = X - 1 alone"""
    g = np.ones(dims, np.uint8)
    g[:, 1, 1] = 0
    g[1:, 5, 1] = 0
    g[dims[0] - 1, 1:6, 1] = 0
    return g


def named_maps():
    """-> list of (name, grid): CPU item 1"""
    X, Y, Z = DIMS
    xs, ys, zs = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    full = np.ones(DIMS, np.uint8)
    corner, edge, two = full.copy(), full.copy(), np.zeros(DIMS, np.uint8)
    corner[7, 7, 7] = corner[8, 8, 8] = 0
    edge[7, 7, 3] = edge[8, 8, 3] = 0
    two[10:14, :, :] = 2   # a slab of byte 2: not enterable, and no obstacle for D2
    two[0, 0, 0] = 1
    return [("empty", np.zeros(DIMS, np.uint8)), ("full", full),
            ("checkerboard", ((xs + ys + zs) % 2).astype(np.uint8)),
            ("even_lattice", (1 - ((xs % 2 == 0) & (ys % 2 == 0) & (zs % 2 == 0))).astype(np.uint8)),
            ("corner_3_borders", corner), ("edge_diagonal", edge), ("serpentine", serpentine()), ("far_end", far_end()),
            ("byte_2", two)]


def degenerate_maps():
    """CPU item 2"""
    rng = np.random.default_rng(7)
    return [("1x1x1", np.zeros((1, 1, 1), np.uint8)), ("9x1x17", (rng.random((9, 1, 17)) < 0.3).astype(np.uint8)),
            ("1024x2x2", np.zeros((1024, 2, 2), np.uint8))]


def random_map(dims, seed):
    """free voxels are those with np.random.default_rng(seed).random(dims) < 0.12"""
    return (1 - (np.random.default_rng(seed).random(dims) < 0.12)).astype(np.uint8)


def random_maps():
    return [("random_%dx%dx%d_seed%d" % (d + (s,)), random_map(d, s)) for d in (DIMS, DIMS_BIG) for s in (1, 2)]


def door_map(width, dims=DIMS):
    """a wall at x = 12 with one square door of `width` voxels in y and z"""
    g = np.zeros(dims, np.uint8)
    g[12] = 1
    y0, z0 = (dims[1] - width) // 2, (dims[2] - width) // 2
    g[12, y0:y0 + width, z0:z0 + width] = 0
    return g


def separating_floor(grid, d2):
    """the smallest min_d2 >= 2 at which (0, 0, 0)'s room no longer reaches the far corner, from the restatement's flood fill"""
    far = tuple(np.array(grid.shape) - 1)
    seeds = np.zeros(grid.shape, bool)
    seeds[0, 0, 0] = True
    for floor in range(2, 200):
        ent = enterable(grid, d2, floor)
        assert ent[0, 0, 0] and ent[far], "the rooms' corners stay enterable"
        if not flood(ent, seeds)[far]:
            return floor
    raise AssertionError("the rooms never separate")


def spans_tiles(label):
    """components that have voxels in two or more 8^3 tiles"""
    X, Y, Z = label.shape
    xs, ys, zs = np.meshgrid(np.arange(X) // 8, np.arange(Y) // 8, np.arange(Z) // 8, indexing="ij")
    tile = (xs * 1000 + ys) * 1000 + zs
    sel = label >= 0
    pairs = np.unique(np.stack([label[sel], tile[sel]], 1), axis=0)
    return int((np.bincount(np.unique(pairs[:, 0], return_inverse=True)[1]) >= 2).sum())


def free_pairs(grid, n, seed, d2=None, min_d2=0):
    """n pairs of enterable voxels"""
    rng = np.random.default_rng(seed)
    vox = np.argwhere(enterable(grid, d2, min_d2)).astype(np.int32)
    return vox[rng.integers(0, len(vox), n)], vox[rng.integers(0, len(vox), n)]


def rule_pairs(grid, n=64, seed=5):
    """CPU item 6: a quarter of the starts on occupied voxels, s == g on an occupied voxel, a goal that is a neighbour of an
    occupied start, endpoints outside the map on each side"""
    rng = np.random.default_rng(seed)
    dims = np.array(grid.shape)
    starts, goals = free_pairs(grid, n, seed)
    occ = np.argwhere(grid != 0).astype(np.int32)
    q = n // 4
    starts[:q] = occ[rng.integers(0, len(occ), q)]
    starts[q] = goals[q] = occ[0]                                   # s == g on an occupied voxel
    for o in occ:                                                   # a goal beside an occupied start
        nb = [o + np.array(d) for d in OFFSETS]
        nb = [v for v in nb if ((v >= 0) & (v < dims)).all() and grid[tuple(v)] == 0]
        if nb:
            starts[q + 1], goals[q + 1] = o, nb[0]
            break
    k = q + 2
    for a in range(3):                                              # outside the map on each side, start and goal
        for val in (-1, dims[a]):
            starts[k, a] = val
            goals[k + 1, a] = val
            k += 2
    return starts, goals


# ---- the header, compiled by g++ ----------------------------------------------------------------------------------------
HARNESS = r'''
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>
#include "free_comp_math.h"
namespace fc = direct::freecomp;

template <typename T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
template <typename T> static void wr(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  // header: X Y Z min_d2 cap2 order n_pairs
  const std::vector<int32_t> hd = rd<int32_t>(fi, 7);
  const int X = hd[0], Y = hd[1], Z = hd[2], min_d2 = hd[3], cap2 = hd[4], order = hd[5], n = hd[6];
  const int G = X * Y * Z;
  const std::vector<uint8_t> map = rd<uint8_t>(fi, G);
  const std::vector<int32_t> d2 = rd<int32_t>(fi, min_d2 > 1 ? G : 0);
  const std::vector<int32_t> starts = rd<int32_t>(fi, 3 * (size_t)n), goals = rd<int32_t>(fi, 3 * (size_t)n);
  fclose(fi);
  FILE* fo = fopen(argv[2], "wb");
  int32_t refused = fc::normal_floor(min_d2) > cap2 ? 1 : 0;   // a stored cap2 means "at least cap2"
  fwrite(&refused, 4, 1, fo);
  if (refused) { fclose(fo); return 0; }
  const int floor = fc::normal_floor(min_d2);
  const auto t0 = std::chrono::steady_clock::now();   // the build on one host thread, for tools/free_comp_bench.py
  std::vector<int32_t> parent(G), size(G, 0);
  int err = 0;
  const int tx = (X + 7) / 8, ty = (Y + 7) / 8, tz = (Z + 7) / 8;
  // ---- k_cc_tile: one workgroup per tile, its lanes one after the other
  for (int t = 0; t < tx * ty * tz; t++) {
    int s_par[fc::kTileVox];
    const int x0 = (t / (ty * tz)) * 8, y0 = ((t / tz) % ty) * 8, z0 = (t % tz) * 8;
    for (int l = 0; l < fc::kTileVox; l++) {
      const int x = x0 + (l >> 6), y = y0 + ((l >> 3) & 7), z = z0 + (l & 7);
      s_par[l] = (x < X && y < Y && z < Z && fc::enterable(map.data(), d2.data(), ((long long)x * Y + y) * Z + z, floor)) ? l : -1;
    }
    auto load = [&](int i) { return s_par[i]; };
    auto amin = [&](int i, int v) { const int old = s_par[i]; if (v < old) s_par[i] = v; return old; };
    for (int l = 0; l < fc::kTileVox; l++) {
      if (s_par[l] < 0) continue;
      const int lx = l >> 6, ly = (l >> 3) & 7, lz = l & 7;
      for (int k = 0; k < fc::kForward; k++) {
        int dx, dy, dz;
        fc::forward_offset(k, dx, dy, dz);
        const int nx = lx + dx, ny = ly + dy, nz = lz + dz;
        if (nx >= 8 || ny < 0 || ny >= 8 || nz < 0 || nz >= 8) continue;
        const int m = (nx << 6) | (ny << 3) | nz;
        if (s_par[m] < 0) continue;
        fc::unite(load, amin, l, m, fc::kTileVox, &err);
      }
    }
    for (int l = 0; l < fc::kTileVox; l++) {
      const int x = x0 + (l >> 6), y = y0 + ((l >> 3) & 7), z = z0 + (l & 7);
      if (x >= X || y >= Y || z >= Z) continue;
      int r = -1;
      if (s_par[l] >= 0) {
        const int q = fc::root_of(load, l, fc::kTileVox, &err);
        r = ((x0 + (q >> 6)) * Y + (y0 + ((q >> 3) & 7))) * Z + (z0 + (q & 7));
      }
      parent[((long long)x * Y + y) * Z + z] = r;
    }
  }
  // ---- k_cc_merge: the unions of all lanes, in the order asked for (0: lane order, 1: reversed, >= 2: shuffled with that seed)
  std::vector<std::pair<int, int>> todo;
  for (int v = 0; v < G; v++) {
    if (parent[v] < 0) continue;
    const int x = v / (Y * Z), y = (v / Z) % Y, z = v % Z;
    for (int k = 0; k < fc::kForward; k++) {
      int dx, dy, dz;
      fc::forward_offset(k, dx, dy, dz);
      const int nx = x + dx, ny = y + dy, nz = z + dz;
      if (nx >= X || ny < 0 || ny >= Y || nz < 0 || nz >= Z) continue;
      if ((nx >> 3) == (x >> 3) && (ny >> 3) == (y >> 3) && (nz >> 3) == (z >> 3)) continue;
      const int m = (nx * Y + ny) * Z + nz;
      if (parent[m] < 0) continue;
      todo.push_back({v, m});
    }
  }
  if (order == 1) std::reverse(todo.begin(), todo.end());
  if (order >= 2) { std::mt19937 gen(order); std::shuffle(todo.begin(), todo.end(), gen); }
  {
    auto load = [&](int i) { return parent[i]; };
    auto amin = [&](int i, int v) { const int old = parent[i]; if (v < old) parent[i] = v; return old; };
    for (const auto& e : todo) fc::unite(load, amin, e.first, e.second, G, &err);
    // ---- k_cc_flatten, k_cc_sizes
    for (int v = 0; v < G; v++) {
      if (parent[v] < 0) continue;
      const int r = fc::root_of(load, v, G, &err);
      parent[v] = r;
      size[r] += 1;
    }
  }
  int64_t ent = 0, comps = 0;
  unsigned long long best = 0;
  for (int v = 0; v < G; v++) {
    const int r = parent[v];
    if (r < 0) continue;
    ent++;
    if (r != v) { size[v] = size[r]; continue; }
    comps++;
    best = std::max(best, fc::stat_key(size[v], r));
  }
  const int64_t us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  const std::vector<int64_t> stats = {ent, comps, fc::stat_size(best), fc::stat_label(best), err, (int64_t)todo.size(), us};
  wr(fo, parent); wr(fo, size); wr(fo, stats);
  // ---- k_reach
  std::vector<int32_t> rtn(n), gl(n), gs(n);
  for (int i = 0; i < n; i++) {
    const int32_t* g = &goals[3 * i];
    rtn[i] = fc::reach_pair(&starts[3 * i], g, X, Y, Z, [&](int v) { return parent[v]; }, &gl[i]);
    gs[i] = gl[i] >= 0 ? size[(g[0] * Y + g[1]) * Z + g[2]] : 0;
  }
  wr(fo, rtn); wr(fo, gl); wr(fo, gs);
  // the staleness key: built at (map 3, field 5)
  const fc::Key plain = {3, 5, 0, 1}, floored = {3, 5, 4, 1}, none = {3, 5, 0, 0};
  const std::vector<int32_t> key = {fc::key_serves(plain, 3, 5), fc::key_serves(plain, 3, 6), fc::key_serves(plain, 4, 5),
                                    fc::key_serves(floored, 3, 5), fc::key_serves(floored, 3, 6), fc::key_serves(floored, 4, 5),
                                    fc::key_serves(none, 3, 5), fc::normal_floor(0), fc::normal_floor(1), fc::normal_floor(2)};
  wr(fo, key);
  fclose(fo);
  return 0;
}
'''


def build(workdir):
    return compile_program(workdir, "free_comp_harness", HARNESS)


def run(exe, grid, d2=None, min_d2=0, cap2=0x7fffffff, order=0, starts=None, goals=None):
    """-> dict(label, size, stats[4], err, unions, host_ms, rtn, goal_label, goal_size, key[10]), or None when the floor is refused"""
    grid = np.ascontiguousarray(grid, np.uint8)
    X, Y, Z = grid.shape
    starts = np.zeros((0, 3), np.int32) if starts is None else np.ascontiguousarray(starts, np.int32).reshape(-1, 3)
    goals = np.zeros((0, 3), np.int32) if goals is None else np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
    n = len(starts)
    fin, fout = exe + ".in", exe + ".out"
    with open(fin, "wb") as f:
        np.array([X, Y, Z, min_d2, cap2, order, n], np.int32).tofile(f)
        grid.tofile(f)
        if min_d2 > 1:
            np.ascontiguousarray(d2, np.int32).tofile(f)
        starts.tofile(f)
        goals.tofile(f)
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        if np.fromfile(f, np.int32, 1)[0]:
            return None
        G = grid.size
        r = dict(label=np.fromfile(f, np.int32, G).reshape(grid.shape), size=np.fromfile(f, np.int32, G).reshape(grid.shape))
        st = np.fromfile(f, np.int64, 7)
        r.update(stats=st[:4].copy(), err=int(st[4]), unions=int(st[5]), host_ms=st[6] / 1e3, rtn=np.fromfile(f, np.int32, n), goal_label=np.fromfile(f, np.int32, n),
                 goal_size=np.fromfile(f, np.int32, n), key=np.fromfile(f, np.int32, 10))
        assert f.read() == b""
    os.remove(fin)
    os.remove(fout)
    assert r["err"] == 0, "a union-find loop passed its trip bound"
    return r


def assert_same(got, want_label, want_size, want_stats, what=""):
    assert got["label"].dtype == np.int32 and got["label"].tobytes() == np.ascontiguousarray(want_label, np.int32).tobytes(), what
    assert got["size"].tobytes() == np.ascontiguousarray(want_size, np.int32).tobytes(), what
    assert np.array_equal(got["stats"], want_stats), (what, got["stats"], want_stats)
