"""g++ build of direct_amd/csrc/grid_path_fan_math.h (which includes grid_path_clear_math.h and grid_path_math.h) as ONE program -
TEST INFRASTRUCTURE of the three tests/test_grid_path*_restatement.py, the three tests/test_gpu_grid_path*.py and the grid path
bench tools.  tests/grid_path_clear_harness.py and tests/grid_path_fan_harness.py are wrappers over this program; its parts are
named after the kernel's (direct_amd/csrc/grid_path.h), to be read next to it.

Shared, written once, by every emulated side (the plain pair, the clear pair, the fan in both modes):
  init   k_path_init: the field at +inf but for the start's 0, the start's tile flagged;
  visit  path_visit<Clear, Fan>, lane after lane: the staged halo, `lim`, `open` and `pen` as the two flags decide them, the sweeps in
         lane order through the header's relax_candidate OR clear_candidate (two branches, never one with a zero penalty: the
         neutral cases of the tests hold them against each other), accept, the write-back with wake_mask, the 27 wakes, and the
         `pending` / `rounds` / `visits` bookkeeping;
  walk   path_walk<Clear, Fan>: the read-back with the header's predecessor rule, or (header == false) with the written-out one;
  the pair driver (rounds until nothing is pending) and the fan driver (counting sort by source, k_fan_bound through the header's
  fan_eligible / fan_bound_fold, the host's batches of rounds, the bound refreshed before every round or every batch);
  one input reader, one record per path, one main.
Independent, on purpose: `dijkstra`, a heap Dijkstra over the whole connected component (full) or left when the goal is popped
(early: the sequential search the stage replaces; its field is exact wherever the true distance is <= the path's cost and an upper
bound elsewhere).  It shares no loop with visit.  In clear mode it is the DEFINED cost written out - two rounded additions per
move, (d(u) + w) + pen(v), the floor on D2, the table indexed here - and its read-back uses the written-out predecessor rule: no
clearance function of the header on that side, so that a mistake in one of them shows as a difference between the sides.  In plain
mode the one addition d(u) + w has nothing to restate; its witness is the Python Dijkstra of tests/test_grid_path_restatement.py.

Three sides per pair query - full, early, emu - with the contract's return codes; the fan has the emulated side alone and is held
against `full` run on every (source, goal) pair.  Also here: the maps and cases the CPU and the GPU tests share."""
import os
import subprocess

import numpy as np

from tests.cpp_program import compile_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NO_PATH, BAD_ENDPOINT, OVERFLOW, ROUND_LIMIT = 0, 1, 2, 3, 4
SIDES = ("full", "early", "emu")   # also the program's side bits and the order of its records within a query

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <vector>
#include "grid_path_fan_math.h"
namespace gp = direct::gridpath;
#ifndef FAN_BOUND_EVERY
#define FAN_BOUND_EVERY 1
#endif
// clear: the map carries D2, a floor and a penalty table (d2 is EMPTY otherwise: plain mode reads neither)
struct Map { int X, Y, Z, YZ, G, tx, ty, tz, nt, clear, min_d2, n_pen; std::vector<uint8_t> m; std::vector<int32_t> d2; std::vector<double> pen; };
static bool inside(const Map& M, int x, int y, int z) { return x >= 0 && x < M.X && y >= 0 && y < M.Y && z >= 0 && z < M.Z; }
static bool inside(const Map& M, const int* p) { return inside(M, p[0], p[1], p[2]); }
static int index_of(const Map& M, const int* p) { return p[0] * M.YZ + p[1] * M.Z + p[2]; }
// one workspace slot: a field with its active flags of two parities and its counters (a pair's, or a fan source's)
struct Field { std::vector<double> d; std::vector<uint8_t> flag[2]; int pending = 0, rounds = 0, visits = 0; };
struct Out { int rtn = 0, len = 0, stats[2] = {0, 0}, min_d2 = 0x7fffffff; double cost = 0.0, ms = 0.0; std::vector<int> path, pd2; };

// ---- the independent side: in clear mode the definition written out, no clearance function of the header ----------------
static double pen_of(const Map& M, int v) { return M.d2[v] < M.n_pen ? M.pen[M.d2[v]] : 0.0; }
static void dijkstra(const Map& M, bool clear, const int* s, const int* g, bool early, std::vector<double>& d) {
  typedef std::pair<double, int> E;
  std::priority_queue<E, std::vector<E>, std::greater<E>> pq;
  const int si = index_of(M, s), gi = index_of(M, g);
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
      if (M.m[u] != 0 || (clear && M.d2[u] < M.min_d2)) continue;
      double c;
      if (clear) {
        volatile double step = d[v] + gp::weight(dx, dy, dz);  // rounded to double before the second addition
        c = step + pen_of(M, u);
      } else {
        c = d[v] + gp::weight(dx, dy, dz);
      }
      if (c < d[u]) { d[u] = c; pq.push(E(c, u)); }
    }
  }
}

// ---- the emulated side ------------------------------------------------------------------------------------------------------
// k_path_init with ends = (start, goal); a fan source passes (source, source)
static void init(const Map& M, Field& F, const int* s, const int* g) {
  F.d.assign(M.G, gp::inf());
  F.flag[0].assign(M.nt, 0);
  F.flag[1].assign(M.nt, 0);
  F.pending = F.rounds = F.visits = 0;
  if (!inside(M, s) || !inside(M, g)) { F.pending = -1; return; }
  F.d[index_of(M, s)] = 0.0;
  F.flag[0][((s[0] / gp::kTile) * M.ty + s[1] / gp::kTile) * M.tz + s[2] / gp::kTile] = 1;
}

// One visit of path_visit<Clear, Fan>, lane t = 0 .. 255 and its voxels j = 0, 1 one after the other.  What the flags decide:
//   lim   !fan: the goal's value read once per visit, or the staged value in every sweep when the goal lies in this tile;
//         fan: fan_bound.
//   open  the voxel's map byte is 0; clear: clear_open as well.
//   pen   clear: clear_penalty, fetched once per visit and voxel; otherwise none - the plain branch is relax_candidate alone.
static void visit(bool clear, bool fan, const Map& M, Field& F, int tile, int round, const int* goal, double fan_bound) {
  std::vector<double>& d = F.d;
  std::vector<uint8_t>&cur = F.flag[round & 1], &nxt = F.flag[(round + 1) & 1];
  static std::vector<double> st(gp::kStaged);
  cur[tile] = 0;
  F.rounds = round + 1;
  F.visits++;
  const int iz = tile % M.tz, iy = (tile / M.tz) % M.ty, ix = tile / (M.tz * M.ty);
  const int bx = ix * gp::kTile, by = iy * gp::kTile, bz = iz * gp::kTile;
  double bound;
  int gl = -1;  // the goal's staged index when it lies in this tile
  if (fan) {
    bound = fan_bound;
  } else {
    bound = d[index_of(M, goal)];
    const int glx = goal[0] - bx, gly = goal[1] - by, glz = goal[2] - bz;
    if (glx >= 0 && glx < gp::kTile && gly >= 0 && gly < gp::kTile && glz >= 0 && glz < gp::kTile)
      gl = gp::staged_index(glx + 1, gly + 1, glz + 1);
  }
  for (int hx = 0; hx < gp::kHalo; hx++)
    for (int hy = 0; hy < gp::kHalo; hy++)
      for (int hz = 0; hz < gp::kHalo; hz++) {
        const int x = bx + hx - 1, y = by + hy - 1, z = bz + hz - 1;
        st[gp::staged_index(hx, hy, hz)] = inside(M, x, y, z) ? d[x * M.YZ + y * M.Z + z] : gp::inf();
      }
  int c[512];        // once per visit and owned voxel, as the kernel's registers
  bool open[512];
  double pen[512];
  for (int t = 0; t < 256; t++)
    for (int j = 0; j < 2; j++) {
      const int lz = t & 7, lx = ((t >> 3) & 3) + 4 * j, ly = t >> 5, x = bx + lx, y = by + ly, z = bz + lz, i = 2 * t + j;
      c[i] = gp::staged_index(lx + 1, ly + 1, lz + 1);
      const bool in = inside(M, x, y, z);
      const int gidx = in ? x * M.YZ + y * M.Z + z : 0;
      if (clear) {
        const int32_t dd = in ? M.d2[gidx] : 0;
        open[i] = in && gp::clear_open(M.m[gidx], dd, M.min_d2);
        pen[i] = open[i] ? gp::clear_penalty(M.pen.data(), M.n_pen, dd) : 0.0;
      } else {
        open[i] = in && M.m[gidx] == 0;
        pen[i] = 0.0;
      }
    }
  int busy = 0;
  for (int it = 0; it < gp::kLocalIters; it++) {
    busy = 0;
    const double lim = gl >= 0 ? st[gl] : bound;
    for (int t = 0; t < 256; t++)
      for (int j = 0; j < 2; j++) {
        const int i = 2 * t + j;
        if (!open[i]) continue;
        const double cand = clear ? gp::clear_candidate(st.data(), c[i], pen[i]) : gp::relax_candidate(st.data(), c[i]);
        if (gp::accept(cand, st[c[i]], lim)) { st[c[i]] = cand; busy = 1; }
      }
    if (!busy) break;
  }
  unsigned wake = busy ? 1u << 13 : 0u;  // the sweeps ran out with changes left: the tile goes on in the next round
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
      if (nx >= 0 && nx < M.tx && ny >= 0 && ny < M.ty && nz >= 0 && nz < M.tz) { nxt[(nx * M.ty + ny) * M.tz + nz] = 1; F.pending = round + 1; }
    }
}

// The read-back of path_walk<Clear, Fan> on a converged field, goal -> start, emitted start -> goal: the first `cap` hops when the
// path is longer (OVERFLOW).  header: the header's is_predecessor / clear_is_predecessor and clear_penalty; otherwise the
// predecessor test and the table look-up written out (the independent side of clear mode).  !clear: path_d2 is 0, no minimum.
static void walk(bool clear, bool header, const Map& M, const int* s, const int* g, const std::vector<double>& d, int cap, Out& o) {
  int x = g[0], y = g[1], z = g[2];
  double dv = d[x * M.YZ + y * M.Z + z];
  o.cost = dv;
  if (!(dv < gp::inf())) { o.rtn = 1; return; }
  std::vector<int> back, bd2;
  for (;;) {
    const int v = x * M.YZ + y * M.Z + z;
    const int32_t dd = clear ? M.d2[v] : 0;
    back.push_back(x); back.push_back(y); back.push_back(z);
    bd2.push_back(dd);
    if (x == s[0] && y == s[1] && z == s[2]) break;
    if (clear && dd < o.min_d2) o.min_d2 = dd;
    const double pen = !clear ? 0.0 : header ? gp::clear_penalty(M.pen.data(), M.n_pen, dd) : pen_of(M, v);
    int k = 0;
    double du = 0.0;
    for (; k < 26; k++) {
      int dx, dy, dz;
      gp::neighbour(k, dx, dy, dz);
      du = inside(M, x + dx, y + dy, z + dz) ? d[(x + dx) * M.YZ + (y + dy) * M.Z + z + dz] : gp::inf();
      if (header) {
        if (clear ? gp::clear_is_predecessor(du, k, pen, dv) : gp::is_predecessor(du, k, dv)) break;
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

static long long round_limit(const Map& M, int max_rounds) { return max_rounds > 0 ? max_rounds : gp::default_max_rounds(M.X, M.Y, M.Z); }

// the pair's rounds, tile after tile; returns 1 when max_rounds ended them with tiles still active
static int pair_rounds(const Map& M, Field& F, const int* g, int max_rounds) {
  const long long lim = round_limit(M, max_rounds);
  int done = 0;
  while (done < lim && F.pending == done) {
    for (int tile = 0; tile < M.nt; tile++)
      if (F.flag[done & 1][tile]) visit(M.clear, false, M, F, tile, done, g, 0.0);
    done++;
  }
  return F.pending == done;
}

// k_fan_bound for source e with the goals order[lo .. hi)
static double bound_of(const Map& M, const int* e, const std::vector<int>& goal, const std::vector<int>& order, int lo, int hi,
                       const std::vector<double>& d) {
  double m = 0.0;
  if (!inside(M, e)) return m;
  for (int i = lo; i < hi; i++) {
    const int* g = &goal[3 * order[i]];
    if (!inside(M, g)) continue;
    const int idx = index_of(M, g);
    const bool self = g[0] == e[0] && g[1] == e[1] && g[2] == e[2];
    if (gp::fan_eligible(self, M.m[idx], M.clear ? M.d2[idx] : 0, M.clear ? M.min_d2 : 0)) m = gp::fan_bound_fold(m, d[idx]);
  }
  return m;
}

// the fan's rounds over all sources; returns the number of rounds done (source s hit ROUND_LIMIT when S[s].pending equals it)
static int fan_rounds(const Map& M, const std::vector<int>& src, const std::vector<int>& goal, const std::vector<int>& gsrc,
                      int max_rounds, std::vector<Field>& S, std::vector<double>& bound) {
  const int ns = (int)S.size(), ng = (int)gsrc.size();
  std::vector<int> off(ns + 1, 0), order(ng);  // the host's grouping: a counting sort by source
  for (int j = 0; j < ng; j++) off[gsrc[j] + 1]++;
  for (int s = 0; s < ns; s++) off[s + 1] += off[s];
  {
    std::vector<int> at(off.begin(), off.end() - 1);
    for (int j = 0; j < ng; j++) order[at[gsrc[j]]++] = j;
  }
  for (int s = 0; s < ns; s++) init(M, S[s], &src[3 * s], &src[3 * s]);
  const long long lim = round_limit(M, max_rounds);
  int done = 0;
  while (done < lim) {  // the host's batches of rounds, enqueued blindly, then one look at `pending`
    const int n = (int)(lim - done < gp::kFanRoundsPerCheck ? lim - done : gp::kFanRoundsPerCheck);
    for (int r = 0; r < n; r++) {
      if (r % FAN_BOUND_EVERY == 0)
        for (int s = 0; s < ns; s++) bound[s] = bound_of(M, &src[3 * s], goal, order, off[s], off[s + 1], S[s].d);
      for (int s = 0; s < ns; s++)
        for (int tile = 0; tile < M.nt; tile++)
          if (S[s].flag[(done + r) & 1][tile]) visit(M.clear, true, M, S[s], tile, done + r, nullptr, bound[s]);
    }
    done += n;
    bool live = false;
    for (int s = 0; s < ns; s++) live |= S[s].pending == done;
    if (!live) break;
  }
  return done;
}

static void write_path(FILE* o, const Out& r) {
  const int head[6] = {r.rtn, r.len, r.stats[0], r.stats[1], r.min_d2, 0};
  const double hd[2] = {r.cost, r.ms};
  fwrite(head, 4, 6, o);
  fwrite(hd, 8, 2, o);
  if (r.path.empty()) return;  // (and fwrite is not to be given the null of an empty vector)
  fwrite(r.path.data(), 4, r.path.size(), o);
  fwrite(r.pd2.data(), 4, r.pd2.size(), o);
}

// in:  int32 X, Y, Z, fan, n_src, n_goal, cap, max_rounds, sides (bit 0 full, 1 early, 2 emu; pairs only), fields, clear, min_d2,
//      n_pen; uint8 map[G]; int32 d2[G] if clear; float64 pen[n_pen]; int32 src[n_src][3], goal[n_goal][3], goal_src[n_goal]
//      (pairs: n_src == n_goal and goal_src[j] == j)
// out: one record per path: int32 rtn, len, stats[2], min_d2, 0; float64 cost, ms; int32 path[n][3], d2[n], n = min(len, cap)
//      pairs: per query, per enabled side in bit order: the record (ms: the side's time), then float64 field[G] if fields
//      fan:   per goal: the record (stats and ms 0); then per source: int32 stats[2]; float64 bound; float64 field[G] if fields
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  volatile double two = 2.0, three = 3.0;  // the weights written as bits are the reference's sqrt(dx*dx + dy*dy + dz*dz)
  if (gp::kW2 != sqrt(two) || gp::kW3 != sqrt(three)) return 4;
  FILE* f = fopen(argv[1], "rb");
  int h[13];
  if (!f || fread(h, 4, 13, f) != 13) return 1;
  Map M;
  M.X = h[0]; M.Y = h[1]; M.Z = h[2]; M.YZ = M.Y * M.Z; M.G = M.X * M.YZ; M.clear = h[10]; M.min_d2 = h[11]; M.n_pen = h[12];
  M.tx = gp::tiles_along(M.X); M.ty = gp::tiles_along(M.Y); M.tz = gp::tiles_along(M.Z); M.nt = M.tx * M.ty * M.tz;
  const int fan = h[3], ns = h[4], ng = h[5], cap = h[6], max_rounds = h[7], sides = h[8], fields = h[9];
  M.m.resize(M.G); M.d2.resize(M.clear ? M.G : 0); M.pen.resize(M.n_pen);
  std::vector<int> src(3 * ns), goal(3 * ng), gsrc(ng);
  auto get = [f](void* p, size_t size, size_t n) { return n == 0 || fread(p, size, n, f) == n; };  // n == 0: p may be null
  if (!get(M.m.data(), 1, M.m.size()) || !get(M.d2.data(), 4, M.d2.size()) || !get(M.pen.data(), 8, M.pen.size()) ||
      !get(src.data(), 4, src.size()) || !get(goal.data(), 4, goal.size()) || !get(gsrc.data(), 4, gsrc.size()))
    return 1;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (fan) {
    std::vector<Field> S(ns);
    std::vector<double> bound(ns, 0.0);
    const int done = fan_rounds(M, src, goal, gsrc, max_rounds, S, bound);
    for (int j = 0; j < ng; j++) {
      const int s = gsrc[j];
      const int *e = &src[3 * s], *g = &goal[3 * j];
      Out r;
      if (!inside(M, e) || !inside(M, g)) { r.rtn = 2; r.cost = nan(""); }
      else if (S[s].pending == done) { r.rtn = 4; r.cost = nan(""); }
      else walk(M.clear, true, M, e, g, S[s].d, cap, r);
      write_path(o, r);
    }
    for (int s = 0; s < ns; s++) {
      const int st[2] = {S[s].rounds, S[s].visits};
      fwrite(st, 4, 2, o);
      fwrite(&bound[s], 8, 1, o);
      if (fields) fwrite(S[s].d.data(), 8, M.G, o);
    }
  } else {
    Field F;
    for (int q = 0; q < ng; q++) {
      const int *s = &src[3 * gsrc[q]], *g = &goal[3 * q];
      for (int side = 0; side < 3; side++) {
        if (!((sides >> side) & 1)) continue;
        const bool emu = side == 2;
        Out r;
        init(M, F, s, g);  // for the Dijkstra sides too: all they need of it is the field at +inf
        const auto t0 = std::chrono::steady_clock::now();
        if (F.pending < 0) {
          r.rtn = 2;
          r.cost = nan("");
        } else if (!emu) {  // the header's predecessor rule in plain mode, the written-out one in clear mode
          dijkstra(M, M.clear, s, g, side == 1, F.d);
          walk(M.clear, !M.clear, M, s, g, F.d, cap, r);
        } else if (pair_rounds(M, F, g, max_rounds)) {
          r.rtn = 4;
          r.cost = nan("");
        } else {
          walk(M.clear, true, M, s, g, F.d, cap, r);
        }
        if (emu) { r.stats[0] = F.rounds; r.stats[1] = F.visits; }
        r.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        write_path(o, r);
        if (fields) fwrite(F.d.data(), 8, M.G, o);
      }
    }
  }
  fclose(o);
  return 0;
}
'''


def build_program(workdir, local_iters=None, bound_every=1):
    """The one build function, keyed by (local_iters, bound_every): two builds with different options in one workdir keep their own
    executables.  local_iters: a build with fewer sweeps per tile visit than the library's (DIRECT_GRIDPATH_LOCAL_ITERS), so that
    small maps reach the branch in which a tile runs out of sweeps and wakes itself; bound_every: 1 or 8, rounds between two
    refreshes of a fan's bound (FAN_BOUND_EVERY; the pair sides do not look at it)"""
    assert bound_every in (1, 8)
    tag = "%s_%d" % ("lib" if local_iters is None else str(local_iters), bound_every)
    defines = ["-DFAN_BOUND_EVERY=%d" % bound_every] + ([] if local_iters is None else ["-DDIRECT_GRIDPATH_LOCAL_ITERS=%d" % local_iters])
    return str(workdir), compile_program(workdir, "grid_path_harness", HARNESS, tail=defines, exe="grid_path_harness_" + tag)


def build(workdir, local_iters=None):
    """the plain module's build: see build_program"""
    return build_program(workdir, local_iters)


def execute(harness, fan, grid, src, goals, goal_src, path_capacity, max_rounds, sides, fields, clear=False, d2=None, min_d2=0,
            penalty=None):
    """writes the program's input file and runs it -> the name of its output file (the caller reads and removes it).  clear: d2
    [like grid], min_d2 and penalty (None: no table) go with the map; otherwise no d2 reaches the program"""
    d, exe = harness
    grid = np.ascontiguousarray(grid, np.uint8)
    pen = np.zeros(0) if penalty is None else np.ascontiguousarray(penalty, np.float64).reshape(-1)
    src = np.ascontiguousarray(src, np.int32).reshape(-1, 3)
    goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
    goal_src = np.ascontiguousarray(goal_src, np.int32).reshape(-1)
    assert len(goal_src) == len(goals) and (len(goals) == 0 or (goal_src.min() >= 0 and goal_src.max() < len(src)))
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        np.array(list(grid.shape) + [int(fan), len(src), len(goals), path_capacity, max_rounds, sum(1 << SIDES.index(s) for s in sides),
                                     int(fields), int(clear), int(min_d2), len(pen)], np.int32).tofile(f)
        grid.tofile(f)
        if clear:
            d2 = np.ascontiguousarray(d2, np.int32)
            assert d2.shape == grid.shape
            d2.tofile(f)
        pen.tofile(f)
        src.tofile(f)
        goals.tofile(f)
        goal_src.tofile(f)
    subprocess.check_call([exe, fin, fout])
    return fout


def new_paths(n):
    """the per-path part of a result, for read_path to fill"""
    return dict(rtn=np.zeros(n, np.int32), path_len=np.zeros(n, np.int32), path_cost=np.zeros(n), stats=np.zeros((n, 2), np.int32),
                ms=np.zeros(n), path_min_d2=np.zeros(n, np.int32), paths=[], path_d2=[])


def read_path(f, path_capacity, r, i):
    """one path record of the program's output into slot i of r (paths and path_d2 are appended: call in order)"""
    head = np.fromfile(f, np.int32, 6)
    r["rtn"][i], r["path_len"][i], r["stats"][i], r["path_min_d2"][i] = head[0], head[1], head[2:4], head[4]
    r["path_cost"][i], r["ms"][i] = np.fromfile(f, np.float64, 2)
    n = min(int(head[1]), path_capacity)
    r["paths"].append(np.fromfile(f, np.int32, 3 * n).reshape(-1, 3))
    r["path_d2"].append(np.fromfile(f, np.int32, n))


def run_pairs(harness, keys, order, grid, starts, goals, path_capacity, max_rounds, fields, **clearance):
    """the pair sides `order` (in the caller's order) -> {side: dict of `keys`}; clearance: execute()'s clear, d2, min_d2, penalty"""
    starts = np.ascontiguousarray(starts, np.int32).reshape(-1, 3)
    nq, G = len(starts), np.asarray(grid).size
    fout = execute(harness, False, grid, starts, goals, np.arange(nq), path_capacity, max_rounds, order, fields, **clearance)
    res = {s: dict(new_paths(nq), dist=np.zeros((nq, G)) if fields else None) for s in order}
    with open(fout, "rb") as f:
        for q in range(nq):
            for s in SIDES:
                if s in order:
                    read_path(f, path_capacity, res[s], q)
                    if fields:
                        res[s]["dist"][q] = np.fromfile(f, np.float64, G)
        assert f.read() == b""
    os.remove(fout)
    return {s: {k: r[k] for k in keys} for s, r in res.items()}


def run(harness, grid, starts, goals, path_capacity=4096, max_rounds=0, sides=("full", "emu"), fields=True):
    """-> {side: dict(rtn, path_len, path_cost, stats, ms, paths: list of [n][3], dist [nq][G] or None)}"""
    return run_pairs(harness, ("rtn", "path_len", "path_cost", "stats", "ms", "paths", "dist"), [s for s in SIDES if s in sides],
                     grid, starts, goals, path_capacity, max_rounds, fields)


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
