"""g++ build of direct_amd/csrc/grid_path_clear_math.h as a program - TEST INFRASTRUCTURE of
tests/test_grid_path_clear_restatement.py, tests/test_gpu_grid_path_clear.py and tools/grid_path_clear_bench.py.  Two sides per
query:
  full   an independent heap Dijkstra over the whole connected component with the DEFINED cost written out here - two rounded
         additions per move, (d(u) + w) + pen(v), the floor on D2, and the predecessor rule with the same two additions - none
         of it through the header's clearance functions;
  emu    a lane-loop emulation of the tiled rounds of grid_path_clear.h: active flags of two parities, the pruning bound, "open"
         and the penalty fetched once per visit and voxel, the header's clear_candidate / accept / wake functions, and the
         header's clear_is_predecessor for the read-back.
A third side, early, is the Dijkstra of full left when the goal is popped: the sequential search the stage replaces, for the
benchmark's 64 queries on the large map (its field is exact wherever the true distance is <= the path's cost).
All report the contract's return codes, path_d2 and path_min_d2.  Also here: a brute-force NumPy distance field and the maps
the CPU and the GPU tests share.  The map builders of tests/grid_path_harness.py are imported, nothing there is changed."""
import os
import subprocess

import numpy as np

from tests import grid_path_harness as gh

ROOT = gh.ROOT
OK, NO_PATH, BAD_ENDPOINT, OVERFLOW, ROUND_LIMIT = gh.OK, gh.NO_PATH, gh.BAD_ENDPOINT, gh.OVERFLOW, gh.ROUND_LIMIT
DIST_NONE = 0x7fffffff
SIDES = ("full", "emu", "early")

HARNESS = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <vector>
#include "grid_path_clear_math.h"
namespace gp = direct::gridpath;
struct Map { int X, Y, Z, YZ, G, min_d2, n_pen; std::vector<uint8_t> m; std::vector<int32_t> d2; std::vector<double> pen; };
static bool inside(const Map& M, int x, int y, int z) { return x >= 0 && x < M.X && y >= 0 && y < M.Y && z >= 0 && z < M.Z; }
struct Out { int rtn = 0, len = 0, stats[2] = {0, 0}, min_d2 = 0x7fffffff; double cost = 0.0; std::vector<int> path, pd2; };

// ---- the independent side: the definition written out, no clearance function of the header ------------------------------
static double pen_of(const Map& M, int v) { return M.d2[v] < M.n_pen ? M.pen[M.d2[v]] : 0.0; }
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
      if (M.m[u] != 0 || M.d2[u] < M.min_d2) continue;
      volatile double step = d[v] + gp::weight(dx, dy, dz);  // rounded to double before the second addition
      const double c = step + pen_of(M, u);
      if (c < d[u]) { d[u] = c; pq.push(E(c, u)); }
    }
  }
}

// ---- the rounds of k_path_clear_relax, tile after tile; returns 1 when max_rounds ended it with tiles still active -------
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
      bool open[512];   // once per visit and owned voxel, as the kernel's registers
      double pen[512];
      for (int t = 0; t < 256; t++)
        for (int j = 0; j < 2; j++) {
          const int lz = t & 7, lx = ((t >> 3) & 3) + 4 * j, ly = t >> 5, x = bx + lx, y = by + ly, z = bz + lz;
          const bool in = inside(M, x, y, z);
          const int gidx = in ? x * M.YZ + y * M.Z + z : 0;
          const int32_t dd = in ? M.d2[gidx] : 0;
          open[2 * t + j] = in && gp::clear_open(M.m[gidx], dd, M.min_d2);
          pen[2 * t + j] = open[2 * t + j] ? gp::clear_penalty(M.pen.data(), M.n_pen, dd) : 0.0;
        }
      int busy = 0;
      for (int it = 0; it < gp::kLocalIters; it++) {
        busy = 0;
        const double limv = gl >= 0 ? st[gl] : bound;
        for (int t = 0; t < 256; t++)
          for (int j = 0; j < 2; j++) {
            if (!open[2 * t + j]) continue;
            const int lz = t & 7, lx = ((t >> 3) & 3) + 4 * j, ly = t >> 5;
            const int c = gp::staged_index(lx + 1, ly + 1, lz + 1);
            const double cand = gp::clear_candidate(st.data(), c, pen[2 * t + j]);
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

// the read-back; header == false: the predecessor test written out (the independent side)
static void trace(const Map& M, const int* s, const int* g, const std::vector<double>& d, int cap, bool header, Out& o) {
  int x = g[0], y = g[1], z = g[2];
  double dv = d[x * M.YZ + y * M.Z + z];
  o.cost = dv;
  if (!(dv < gp::inf())) { o.rtn = 1; return; }
  std::vector<int> back, bd2;
  for (;;) {
    const int v = x * M.YZ + y * M.Z + z;
    back.push_back(x); back.push_back(y); back.push_back(z);
    bd2.push_back(M.d2[v]);
    if (x == s[0] && y == s[1] && z == s[2]) break;
    if (M.d2[v] < o.min_d2) o.min_d2 = M.d2[v];
    const double pen = header ? gp::clear_penalty(M.pen.data(), M.n_pen, M.d2[v]) : pen_of(M, v);
    int k = 0;
    double du = 0.0;
    for (; k < 26; k++) {
      int dx, dy, dz;
      gp::neighbour(k, dx, dy, dz);
      du = inside(M, x + dx, y + dy, z + dz) ? d[(x + dx) * M.YZ + (y + dy) * M.Z + z + dz] : gp::inf();
      if (header) {
        if (gp::clear_is_predecessor(du, k, pen, dv)) break;
      } else {
        volatile double step = du + gp::weight(dx, dy, dz);
        if (step + pen == dv) break;
      }
    }
    if (k == 26) { fprintf(stderr, "no predecessor\n"); exit(3); }
    int dx, dy, dz;
    gp::neighbour(k, dx, dy, dz);
    x += dx; y += dy; z += dz;
    dv = du;
  }
  o.len = (int)back.size() / 3;
  o.rtn = o.len > cap ? 3 : 0;
  for (int i = 0; i < o.len && i < cap; i++) {
    for (int a = 0; a < 3; a++) o.path.push_back(back[3 * (o.len - 1 - i) + a]);
    o.pd2.push_back(bd2[o.len - 1 - i]);
  }
}

// in: int32 X, Y, Z, nq, cap, max_rounds, sides (bit 0 full, 1 emu, 2 early), fields, min_d2, n_pen; uint8 map[G]; int32 d2[G];
//     float64 pen[n_pen]; int32 starts[nq][3], goals[nq][3]
// out: per query, per enabled side in that order: int32 rtn, len, stats[2], min_d2, 0; float64 cost; int32 path[n][3], d2[n],
//      n = min(len, cap); float64 field[G] if fields
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[10];
  if (!f || fread(h, 4, 10, f) != 10) return 1;
  Map M;
  M.X = h[0]; M.Y = h[1]; M.Z = h[2]; M.YZ = M.Y * M.Z; M.G = M.X * M.YZ; M.min_d2 = h[8]; M.n_pen = h[9];
  const int nq = h[3], cap = h[4], max_rounds = h[5], sides = h[6], fields = h[7];
  M.m.resize(M.G); M.d2.resize(M.G); M.pen.resize(M.n_pen);
  std::vector<int> S(3 * nq), Gl(3 * nq);
  if (fread(M.m.data(), 1, M.G, f) != (size_t)M.G || fread(M.d2.data(), 4, M.G, f) != (size_t)M.G ||
      fread(M.pen.data(), 8, M.n_pen, f) != (size_t)M.n_pen || fread(S.data(), 4, S.size(), f) != S.size() ||
      fread(Gl.data(), 4, Gl.size(), f) != Gl.size())
    return 1;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  std::vector<double> d(M.G);
  for (int q = 0; q < nq; q++) {
    const int *s = &S[3 * q], *g = &Gl[3 * q];
    for (int side = 0; side < 3; side++) {
      if (!((sides >> side) & 1)) continue;
      Out r;
      std::fill(d.begin(), d.end(), gp::inf());
      if (!inside(M, s[0], s[1], s[2]) || !inside(M, g[0], g[1], g[2])) {
        r.rtn = 2;
        r.cost = nan("");
      } else if (side != 1) {
        dijkstra(M, s, g, side == 2, d);
        trace(M, s, g, d, cap, false, r);
      } else if (emulate(M, s, g, max_rounds, d, r.stats)) {
        r.rtn = 4;
        r.cost = nan("");
      } else {
        trace(M, s, g, d, cap, true, r);
      }
      if (r.rtn == 1 || r.rtn == 2 || r.rtn == 4) r.min_d2 = 0x7fffffff;
      const int head[6] = {r.rtn, r.len, r.stats[0], r.stats[1], r.min_d2, 0};
      fwrite(head, 4, 6, o);
      fwrite(&r.cost, 8, 1, o);
      fwrite(r.path.data(), 4, r.path.size(), o);
      fwrite(r.pd2.data(), 4, r.pd2.size(), o);
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
    src = os.path.join(str(workdir), "grid_path_clear_harness.cpp")
    exe = os.path.join(str(workdir), "grid_path_clear_harness" + ("" if local_iters is None else "_%d" % local_iters))
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "direct_amd", "csrc"), src, "-o", exe]
                          + ([] if local_iters is None else ["-DDIRECT_GRIDPATH_LOCAL_ITERS=%d" % local_iters]))
    return str(workdir), exe


def run(harness, grid, d2, starts, goals, min_d2=0, penalty=None, path_capacity=4096, max_rounds=0, sides=("full", "emu"), fields=True):
    """-> {side: dict(rtn, path_len, path_cost, stats, path_min_d2, paths: list of [n][3], path_d2: list of [n], dist [nq][G] or None)}"""
    d, exe = harness
    grid = np.ascontiguousarray(grid, np.uint8)
    d2 = np.ascontiguousarray(d2, np.int32)
    assert d2.shape == grid.shape
    pen = np.zeros(0) if penalty is None else np.ascontiguousarray(penalty, np.float64).reshape(-1)
    starts = np.ascontiguousarray(starts, np.int32).reshape(-1, 3)
    goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
    nq, G = len(starts), grid.size
    mask = sum(1 << SIDES.index(s) for s in sides)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        np.array(list(grid.shape) + [nq, path_capacity, max_rounds, mask, int(fields), int(min_d2), len(pen)], np.int32).tofile(f)
        grid.tofile(f)
        d2.tofile(f)
        pen.tofile(f)
        starts.tofile(f)
        goals.tofile(f)
    subprocess.check_call([exe, fin, fout])
    order = [s for s in SIDES if s in sides]
    res = {s: dict(rtn=np.zeros(nq, np.int32), path_len=np.zeros(nq, np.int32), path_cost=np.zeros(nq), stats=np.zeros((nq, 2), np.int32),
                   path_min_d2=np.zeros(nq, np.int32), paths=[], path_d2=[], dist=np.zeros((nq, G)) if fields else None) for s in order}
    with open(fout, "rb") as f:
        for q in range(nq):
            for s in order:
                r = res[s]
                head = np.fromfile(f, np.int32, 6)
                r["rtn"][q], r["path_len"][q], r["stats"][q], r["path_min_d2"][q] = head[0], head[1], head[2:4], head[4]
                r["path_cost"][q] = np.fromfile(f, np.float64, 1)[0]
                n = min(int(head[1]), path_capacity)
                r["paths"].append(np.fromfile(f, np.int32, 3 * n).reshape(-1, 3))
                r["path_d2"].append(np.fromfile(f, np.int32, n))
                if fields:
                    r["dist"][q] = np.fromfile(f, np.float64, G)
        assert f.read() == b""
    os.remove(fout)
    return res


def brute_distance_field(grid, cap_vox=0):
    """min(D2, cap2) by brute force: for every voxel the smallest squared distance to a voxel with byte 1 (int32, DIST_NONE on a
    map without one; cap2 = cap_vox^2, or none for cap_vox == 0) - the definition of direct_cluster_distance_field"""
    grid = np.asarray(grid)
    occ = np.argwhere(grid == 1).astype(np.int64)
    out = np.full(grid.size, DIST_NONE, np.int64)
    if len(occ):
        vox = np.stack(np.unravel_index(np.arange(grid.size), grid.shape), axis=1).astype(np.int64)
        for a in range(0, len(vox), 512):
            diff = vox[a:a + 512, None, :] - occ[None, :, :]
            out[a:a + 512] = (diff * diff).sum(axis=2).min(axis=1)
    if cap_vox > 0:
        out = np.minimum(out, cap_vox * cap_vox)
    return out.reshape(grid.shape).astype(np.int32)


# ---- the maps the CPU and the GPU tests share: 40 x 24 x 12, five tiles along x, partial tiles along z -----------------------

def walls_map():
    """walls across x, full height, seven voxels apart, each with a gap 7 voxels wide along y (its middle column has D2 = 16) and
    the first four with a second, narrower gap of width 1, 2, 3 and 5 (middle D2 = 1, 1, 4, 9) elsewhere: a floor on D2 closes the
    narrow gaps one after the other and the paths move to the wide ones"""
    g = np.zeros((40, 24, 12), np.uint8)
    for x, wide, narrow in ((6, 15, (3, 1)), (13, 1, (18, 2)), (20, 14, (4, 3)), (27, 2, (17, 5)), (34, 10, None)):
        g[x, :, :] = 1
        g[x, wide:wide + 7, :] = 0
        if narrow:
            g[x, narrow[0]:narrow[0] + narrow[1], :] = 0
    g[0:3, 0, 0] = 1   # a clutter row next to the corner: voxels below a floor that are not walls
    return g


def gap_map():
    """one thick wall across x with a direct gap one voxel wide (y = 12, full height) and a wide opening far off (y = 0 .. 4):
    the unpenalised optimum squeezes through the gap, a proximity penalty pays for the detour through open space"""
    g = np.zeros((40, 24, 12), np.uint8)
    g[18:22, :, :] = 1
    g[18:22, 12, :] = 0
    g[18:22, 0:5, :] = 0
    g[8, 8:16, 3:9] = 1    # two plates the paths skirt on either side of the wall
    g[31, 9:17, 2:8] = 1
    return g


def queries(grid, d2, n, seed, floor=0):
    """n (start, goal) pairs of free voxels with D2 >= floor on opposite sides of the map along x"""
    rng = np.random.default_rng(seed)
    ok = (grid == 0) & (d2 >= floor)
    left, right = np.argwhere(ok[:5]), np.argwhere(ok[35:]) + [35, 0, 0]
    s, g = left[rng.integers(len(left), size=n)], right[rng.integers(len(right), size=n)]
    swap = rng.random(n) < 0.5
    s[swap], g[swap] = g[swap].copy(), s[swap].copy()
    return s.astype(np.int32), g.astype(np.int32)


def soft_table(weight=0.3, radius=4.0):
    """the table of the penalty cases: weight * (1 - sqrt(d2) / radius)^2 below radius^2, non-representable doubles"""
    d2 = np.arange(int(np.ceil(radius * radius)), dtype=np.float64)
    return weight * (1.0 - np.sqrt(d2) / radius) ** 2
