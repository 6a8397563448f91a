"""g++ build of direct_amd/csrc/grid_path_math.h as a program - TEST INFRASTRUCTURE of tests/test_grid_path_restatement.py,
tests/test_gpu_grid_path.py and tools/grid_path_bench.py.  Three sides per query, each with the header's weights:
  full   a heap Dijkstra over the whole connected component (the exact side),
  early  the same Dijkstra left when the goal is popped (the sequential search the stage replaces; its field is exact wherever
         the true distance is <= the path's cost and an upper bound elsewhere, which is what the contract asks of `dist`),
  emu    a lane-loop emulation of the tiled rounds of grid_path.h: active flags of two parities, the pruning bound, the
         header's relax / accept / wake functions, one tile after the other.
All three read the path back with the header's predecessor rule and report the contract's return codes."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NO_PATH, BAD_ENDPOINT, OVERFLOW, ROUND_LIMIT = 0, 1, 2, 3, 4
SIDES = ("full", "early", "emu")

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <vector>
#include "grid_path_math.h"
namespace gp = direct::gridpath;
struct Map { int X, Y, Z, YZ, G; std::vector<uint8_t> m; };
static bool inside(const Map& M, int x, int y, int z) { return x >= 0 && x < M.X && y >= 0 && y < M.Y && z >= 0 && z < M.Z; }
struct Out { int rtn = 0, len = 0, stats[2] = {0, 0}; double cost = 0.0, ms = 0.0; std::vector<int> path; };

static void dijkstra(const Map& M, const int* s, const int* g, bool early, std::vector<double>& d) {
  typedef std::pair<double, int> E;
  std::priority_queue<E, std::vector<E>, std::greater<E>> pq;
  const int si = s[0] * M.YZ + s[1] * M.Z + s[2], gi = g[0] * M.YZ + g[1] * M.Z + g[2];
  d[si] = 0.0;
  pq.push(E(0.0, si));
  while (!pq.empty()) {
    const E t = pq.top();
    pq.pop();
    const int v = t.second;
    if (t.first != d[v]) continue;
    if (early && v == gi) break;
    const int x = v / M.YZ, y = (v / M.Z) % M.Y, z = v % M.Z;
    for (int k = 0; k < 26; k++) {
      int dx, dy, dz;
      gp::neighbour(k, dx, dy, dz);
      const int ux = x + dx, uy = y + dy, uz = z + dz;
      if (!inside(M, ux, uy, uz)) continue;
      const int u = ux * M.YZ + uy * M.Z + uz;
      if (M.m[u] != 0) continue;
      const double c = d[v] + gp::weight(dx, dy, dz);
      if (c < d[u]) { d[u] = c; pq.push(E(c, u)); }
    }
  }
}

// the rounds of k_path_relax, tile after tile; returns 1 when max_rounds ended it with tiles still active
static int emulate(const Map& M, const int* s, const int* g, long long max_rounds, std::vector<double>& d, int* stats) {
  const int tx = gp::tiles_along(M.X), ty = gp::tiles_along(M.Y), tz = gp::tiles_along(M.Z), nt = tx * ty * tz;
  std::vector<uint8_t> flag[2] = {std::vector<uint8_t>(nt, 0), std::vector<uint8_t>(nt, 0)};
  d[s[0] * M.YZ + s[1] * M.Z + s[2]] = 0.0;
  flag[0][((s[0] / gp::kTile) * ty + s[1] / gp::kTile) * tz + s[2] / gp::kTile] = 1;
  const int gi = g[0] * M.YZ + g[1] * M.Z + g[2];
  std::vector<double> st(gp::kStaged);
  int pending = 0, done = 0;
  const long long lim = max_rounds > 0 ? max_rounds : gp::default_max_rounds(M.X, M.Y, M.Z);
  while (done < lim && pending == done) {
    const int round = done;
    std::vector<uint8_t>&cur = flag[round & 1], &nxt = flag[(round + 1) & 1];
    for (int tile = 0; tile < nt; tile++) {
      if (!cur[tile]) continue;
      cur[tile] = 0;
      stats[0] = round + 1;
      stats[1]++;
      const int iz = tile % tz, iy = (tile / tz) % ty, ix = tile / (tz * ty);
      const int bx = ix * gp::kTile, by = iy * gp::kTile, bz = iz * gp::kTile;
      const double bound = d[gi];
      const int glx = g[0] - bx, gly = g[1] - by, glz = g[2] - bz;
      const int gl = (glx >= 0 && glx < gp::kTile && gly >= 0 && gly < gp::kTile && glz >= 0 && glz < gp::kTile)
                         ? gp::staged_index(glx + 1, gly + 1, glz + 1) : -1;
      for (int hx = 0; hx < gp::kHalo; hx++)
        for (int hy = 0; hy < gp::kHalo; hy++)
          for (int hz = 0; hz < gp::kHalo; hz++) {
            const int x = bx + hx - 1, y = by + hy - 1, z = bz + hz - 1;
            st[gp::staged_index(hx, hy, hz)] = inside(M, x, y, z) ? d[x * M.YZ + y * M.Z + z] : gp::inf();
          }
      int busy = 0;
      for (int it = 0; it < gp::kLocalIters; it++) {
        busy = 0;
        const double limv = gl >= 0 ? st[gl] : bound;
        for (int t = 0; t < 256; t++)
          for (int j = 0; j < 2; j++) {
            const int lz = t & 7, lx = ((t >> 3) & 3) + 4 * j, ly = t >> 5, x = bx + lx, y = by + ly, z = bz + lz;
            if (!inside(M, x, y, z) || M.m[x * M.YZ + y * M.Z + z] != 0) continue;
            const int c = gp::staged_index(lx + 1, ly + 1, lz + 1);
            const double cand = gp::relax_candidate(st.data(), c);
            if (gp::accept(cand, st[c], limv)) { st[c] = cand; busy = 1; }
          }
        if (!busy) break;
      }
      unsigned wake = busy ? 1u << 13 : 0u;
      for (int lx = 0; lx < gp::kTile; lx++)
        for (int ly = 0; ly < gp::kTile; ly++)
          for (int lz = 0; lz < gp::kTile; lz++) {
            const int x = bx + lx, y = by + ly, z = bz + lz;
            if (!inside(M, x, y, z)) continue;
            const double v = st[gp::staged_index(lx + 1, ly + 1, lz + 1)];
            if (v != d[x * M.YZ + y * M.Z + z]) { d[x * M.YZ + y * M.Z + z] = v; wake |= gp::wake_mask(lx, ly, lz); }
          }
      for (int b = 0; b < 27; b++)
        if ((wake >> b) & 1u) {
          const int nx = ix + b / 9 - 1, ny = iy + (b / 3) % 3 - 1, nz = iz + b % 3 - 1;
          if (nx >= 0 && nx < tx && ny >= 0 && ny < ty && nz >= 0 && nz < tz) { nxt[(nx * ty + ny) * tz + nz] = 1; pending = round + 1; }
        }
    }
    done++;
  }
  return pending == done;
}

static void trace(const Map& M, const int* s, const int* g, const std::vector<double>& d, int cap, Out& o) {
  int x = g[0], y = g[1], z = g[2];
  double dv = d[x * M.YZ + y * M.Z + z];
  o.cost = dv;
  if (!(dv < gp::inf())) { o.rtn = 1; return; }
  std::vector<int> back;
  for (;;) {
    back.push_back(x); back.push_back(y); back.push_back(z);
    if (x == s[0] && y == s[1] && z == s[2]) break;
    int k = 0;
    double du = 0.0;
    for (; k < 26; k++) {
      int dx, dy, dz;
      gp::neighbour(k, dx, dy, dz);
      du = inside(M, x + dx, y + dy, z + dz) ? d[(x + dx) * M.YZ + (y + dy) * M.Z + z + dz] : gp::inf();
      if (gp::is_predecessor(du, k, dv)) break;
    }
    if (k == 26) { fprintf(stderr, "no predecessor\n"); exit(3); }
    int dx, dy, dz;
    gp::neighbour(k, dx, dy, dz);
    x += dx; y += dy; z += dz;
    dv = du;
  }
  o.len = (int)back.size() / 3;
  o.rtn = o.len > cap ? 3 : 0;
  for (int i = 0; i < o.len && i < cap; i++)
    for (int a = 0; a < 3; a++) o.path.push_back(back[3 * (o.len - 1 - i) + a]);
}

// in: int32 X, Y, Z, nq, cap, max_rounds, sides (bit 0 full, 1 early, 2 emu), fields; uint8 map[G]; int32 starts[nq][3], goals[nq][3]
// out: per query, per enabled side in that order: int32 rtn, len, stats[2]; float64 cost, ms; int32 path[min(len, cap)][3]; float64 field[G] if fields
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  volatile double two = 2.0, three = 3.0;  // the weights written as bits are the reference's sqrt(dx*dx + dy*dy + dz*dz)
  if (gp::kW2 != sqrt(two) || gp::kW3 != sqrt(three)) return 4;
  FILE* f = fopen(argv[1], "rb");
  int h[8];
  if (!f || fread(h, 4, 8, f) != 8) return 1;
  Map M;
  M.X = h[0]; M.Y = h[1]; M.Z = h[2]; M.YZ = M.Y * M.Z; M.G = M.X * M.YZ;
  const int nq = h[3], cap = h[4], max_rounds = h[5], sides = h[6], fields = h[7];
  M.m.resize(M.G);
  std::vector<int> S(3 * nq), Gl(3 * nq);
  if (fread(M.m.data(), 1, M.G, f) != (size_t)M.G || fread(S.data(), 4, S.size(), f) != S.size() || fread(Gl.data(), 4, Gl.size(), f) != Gl.size()) return 1;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  std::vector<double> d(M.G);
  for (int q = 0; q < nq; q++) {
    const int *s = &S[3 * q], *g = &Gl[3 * q];
    for (int side = 0; side < 3; side++) {
      if (!((sides >> side) & 1)) continue;
      Out r;
      std::fill(d.begin(), d.end(), gp::inf());
      const auto t0 = std::chrono::steady_clock::now();
      if (!inside(M, s[0], s[1], s[2]) || !inside(M, g[0], g[1], g[2])) {
        r.rtn = 2;
        r.cost = nan("");
      } else if (side < 2) {
        dijkstra(M, s, g, side == 1, d);
        trace(M, s, g, d, cap, r);
      } else if (emulate(M, s, g, max_rounds, d, r.stats)) {
        r.rtn = 4;
        r.cost = nan("");
      } else {
        trace(M, s, g, d, cap, r);
      }
      r.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      const int head[4] = {r.rtn, r.len, r.stats[0], r.stats[1]};
      const double hd[2] = {r.cost, r.ms};
      fwrite(head, 4, 4, o);
      fwrite(hd, 8, 2, o);
      fwrite(r.path.data(), 4, r.path.size(), o);
      if (fields) fwrite(d.data(), 8, d.size(), o);
    }
  }
  fclose(o);
  return 0;
}
'''


def build(workdir, local_iters=None):
    """local_iters: a build with fewer sweeps per tile visit than the library's (DIRECT_GRIDPATH_LOCAL_ITERS), so that small maps
    reach the branch in which a tile runs out of sweeps and wakes itself"""
    src = os.path.join(str(workdir), "grid_path_harness.cpp")
    exe = os.path.join(str(workdir), "grid_path_harness" + ("" if local_iters is None else "_%d" % local_iters))
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "direct_amd", "csrc"), src, "-o", exe]
                          + ([] if local_iters is None else ["-DDIRECT_GRIDPATH_LOCAL_ITERS=%d" % local_iters]))
    return str(workdir), exe


def run(harness, grid, starts, goals, path_capacity=4096, max_rounds=0, sides=("full", "emu"), fields=True):
    """-> {side: dict(rtn, path_len, path_cost, stats, ms, paths: list of [n][3], dist [nq][G] or None)}"""
    d, exe = harness
    grid = np.ascontiguousarray(grid, np.uint8)
    starts = np.ascontiguousarray(starts, np.int32).reshape(-1, 3)
    goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
    nq, G = len(starts), grid.size
    mask = sum(1 << SIDES.index(s) for s in sides)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        np.array(list(grid.shape) + [nq, path_capacity, max_rounds, mask, int(fields)], np.int32).tofile(f)
        grid.tofile(f)
        starts.tofile(f)
        goals.tofile(f)
    subprocess.check_call([exe, fin, fout])
    order = [s for s in SIDES if s in sides]
    res = {s: dict(rtn=np.zeros(nq, np.int32), path_len=np.zeros(nq, np.int32), path_cost=np.zeros(nq), stats=np.zeros((nq, 2), np.int32),
                   ms=np.zeros(nq), paths=[], dist=np.zeros((nq, G)) if fields else None) for s in order}
    with open(fout, "rb") as f:
        for q in range(nq):
            for s in order:
                r = res[s]
                head = np.fromfile(f, np.int32, 4)
                hd = np.fromfile(f, np.float64, 2)
                r["rtn"][q], r["path_len"][q], r["stats"][q] = head[0], head[1], head[2:]
                r["path_cost"][q], r["ms"][q] = hd
                r["paths"].append(np.fromfile(f, np.int32, 3 * min(int(head[1]), path_capacity)).reshape(-1, 3))
                if fields:
                    r["dist"][q] = np.fromfile(f, np.float64, G)
        assert f.read() == b""
    os.remove(fout)
    return res


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------

def big_map():
    from direct_amd import problems
    grid, _ = problems.make_voxel_map((200, 200, 40), seed=7, n_pillars=170, n_boxes=70, n_rings=12)
    return np.ascontiguousarray(grid, np.uint8)


def big_queries(grid, n):
    """Endpoint pairs drawn as tests/real_corridor_lib.real_corridor_batch draws them: both free, in one z-slice, |delta|_1 > 120,
    connected inside the slice (so that the 4-connected path of that file exists for comparison)"""
    from tests.real_corridor_lib import grid_path
    rng = np.random.default_rng(5)
    starts, goals = [], []
    while len(starts) < n:
        z = int(rng.integers(4, 30))
        free = np.argwhere(grid[:, :, z] == 0)
        a, b = free[rng.integers(len(free))], free[rng.integers(len(free))]
        if np.abs(a - b).sum() > 120 and grid_path(grid, [a[0], a[1], z], [b[0], b[1], z]) is not None:
            starts.append([a[0], a[1], z])
            goals.append([b[0], b[1], z])
    return np.array(starts, np.int32), np.array(goals, np.int32)


def random_map(dims, seed, density=0.25):
    rng = np.random.default_rng(seed)
    return (rng.random(dims) < density).astype(np.uint8)


def sealed_box_map():
    g = np.zeros((20, 18, 12), np.uint8)
    g[4:11, 5:12, 2:9] = 1     # a closed shell ...
    g[5:10, 6:11, 3:8] = 0     # ... around a free 5 x 5 x 5 room
    return g


def maze_map():
    """serpentine walls across x, full height, with a one-voxel-wide gap at alternating ends of y"""
    g = np.zeros((32, 24, 12), np.uint8)
    for i, x in enumerate(range(2, 31, 3)):
        g[x, :, :] = 1
        if i % 2:
            g[x, 0, :] = 0
        else:
            g[x, 23, :] = 0
    return g


def tile_serpentine_map():
    """ONE 8^3 tile filled by a serpentine of about 140 hops: free layers z = 0, 2, 4, 6 joined by one hole in each wall layer
    between them, and inside a free layer the rows y = 0, 2, 4, 6 joined by one gap at alternating ends of the wall rows.  A sweep
    of the kernel moves a value one hop where the lanes' values meet stale ones, so 64 sweeps do not finish the tile: its visit
    runs out of sweeps and the tile wakes ITSELF (it has no neighbour that could)."""
    g = np.ones((8, 8, 8), np.uint8)
    for i, z in enumerate((0, 2, 4, 6)):
        for j, y in enumerate((0, 2, 4, 6)):
            g[:, y, z] = 0
            if j < 3:
                g[7 if j % 2 == 0 else 0, y + 1, z] = 0
        if i < 3:  # an even layer is walked from row y = 0 to row 6, an odd one back from 6 to 0; both end at x = 0
            g[0, 6 if i % 2 == 0 else 0, z + 1] = 0
    return g


def crafted_cases():
    """-> list of dict(name, grid, starts, goals, cap, max_rounds, rtn): every return code of the contract, partial tiles, a 2-D
    map, the maze, an occupied start, start == goal, a path_capacity that is too small and the round cap"""
    cases = []
    g = random_map((13, 11, 5), 11, 0.2)
    g[0, 0, 0] = 0; g[12, 10, 4] = 0; g[6, 5, 2] = 1; g[7, 7, 3] = 1; g[1, 1, 1] = 0
    cases.append(dict(name="partial_tiles", grid=g, cap=64, max_rounds=0,
                      starts=[[0, 0, 0], [12, 10, 4], [3, 3, 3], [6, 5, 2], [0, 0, 0], [-1, 0, 0], [0, 0, 0], [6, 5, 2]],
                      goals=[[12, 10, 4], [0, 0, 0], [3, 3, 3], [12, 10, 4], [7, 7, 3], [1, 1, 1], [0, 11, 0], [6, 5, 2]],
                      rtn=[OK, OK, OK, OK, NO_PATH, BAD_ENDPOINT, BAD_ENDPOINT, OK]))
    cases.append(dict(name="capacity", grid=g, cap=3, max_rounds=0, starts=[[0, 0, 0], [1, 1, 1]], goals=[[12, 10, 4], [0, 0, 0]],
                      rtn=[OVERFLOW, OK]))
    b = sealed_box_map()
    cases.append(dict(name="sealed_box", grid=b, cap=64, max_rounds=0, starts=[[7, 8, 5], [7, 8, 5], [0, 0, 0]],
                      goals=[[18, 16, 10], [9, 10, 7], [7, 8, 5]], rtn=[NO_PATH, OK, NO_PATH]))
    f = random_map((32, 24, 1), 3, 0.3)
    f[0, 0, 0] = 0; f[31, 23, 0] = 0; f[31, 0, 0] = 0
    cases.append(dict(name="flat", grid=f, cap=128, max_rounds=0, starts=[[0, 0, 0], [31, 0, 0]], goals=[[31, 23, 0], [0, 0, 0]], rtn=None))
    m = maze_map()
    cases.append(dict(name="maze", grid=m, cap=512, max_rounds=0, starts=[[0, 0, 0], [31, 23, 11]], goals=[[31, 23, 11], [0, 12, 5]], rtn=[OK, OK]))
    cases.append(dict(name="round_limit", grid=m, cap=512, max_rounds=1, starts=[[0, 0, 0], [4, 4, 4], [0, 0, 0]],
                      goals=[[31, 23, 11], [4, 4, 4], [31, 23, 11]], rtn=[ROUND_LIMIT, OK, ROUND_LIMIT]))
    cases.append(dict(name="tile_serpentine", grid=tile_serpentine_map(), cap=512, max_rounds=0, starts=[[0, 0, 0], [0, 0, 0]],
                      goals=[[0, 0, 6], [7, 0, 6]], rtn=[OK, OK]))
    for c in cases:
        c["starts"], c["goals"] = np.array(c["starts"], np.int32), np.array(c["goals"], np.int32)
    return cases
