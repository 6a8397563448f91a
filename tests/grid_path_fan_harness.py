"""g++ build of direct_amd/csrc/grid_path_fan_math.h as a program - TEST INFRASTRUCTURE of tests/test_grid_path_fan_restatement.py
and tests/test_gpu_grid_path_fan.py.  ONE side: a lane-loop emulation of the rounds of grid_path_fan.h - one field per source, the
bound of a source as k_fan_bound makes it (the header's fan_eligible / fan_bound_fold over the source's goals), refreshed before
every round or before every batch of eight (a build option, as the sweeps per visit), k_fan_relax's visit with lim = bound[s]
through the header's relax_candidate / clear_candidate / accept / wake_mask, the host's batches of eight rounds, and one read-back
per goal with the header's predecessor rules.  The independent side is NOT here: the tests hold every goal against the heap
Dijkstra of tests/grid_path_harness.py (neutral mode) and tests/grid_path_clear_harness.py (clear mode), run on the pair; those
modules are imported, nothing in them is changed."""
import os
import subprocess

import numpy as np

from tests import grid_path_harness as gh

ROOT = gh.ROOT
OK, NO_PATH, BAD_ENDPOINT, OVERFLOW, ROUND_LIMIT = gh.OK, gh.NO_PATH, gh.BAD_ENDPOINT, gh.OVERFLOW, gh.ROUND_LIMIT
DIST_NONE = 0x7fffffff

HARNESS = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "grid_path_fan_math.h"
namespace gp = direct::gridpath;
#ifndef FAN_BOUND_EVERY
#define FAN_BOUND_EVERY 1
#endif
struct Map { int X, Y, Z, YZ, G, clear, min_d2, n_pen; std::vector<uint8_t> m; std::vector<int32_t> d2; std::vector<double> pen; };
static bool inside(const Map& M, const int* p) { return p[0] >= 0 && p[0] < M.X && p[1] >= 0 && p[1] < M.Y && p[2] >= 0 && p[2] < M.Z; }
static bool inside(const Map& M, int x, int y, int z) { const int p[3] = {x, y, z}; return inside(M, p); }
struct Fan { int ns, ng; std::vector<int> src, goal, gsrc, order, off; };

// k_fan_bound for source s
static double bound_of(const Map& M, const Fan& F, int s, const std::vector<double>& d) {
  const int* e = &F.src[3 * s];
  double m = 0.0;
  if (!inside(M, e)) return m;
  for (int i = F.off[s]; i < F.off[s + 1]; i++) {
    const int* g = &F.goal[3 * F.order[i]];
    if (!inside(M, g)) continue;
    const int idx = g[0] * M.YZ + g[1] * M.Z + g[2];
    const bool self = g[0] == e[0] && g[1] == e[1] && g[2] == e[2];
    if (gp::fan_eligible(self, M.m[idx], M.clear ? M.d2[idx] : 0, M.clear ? M.min_d2 : 0)) m = gp::fan_bound_fold(m, d[idx]);
  }
  return m;
}

struct Src { std::vector<double> d; std::vector<uint8_t> flag[2]; int pending = 0, rounds = 0, visits = 0; double bound = 0.0; };

// one visit of k_fan_relax
static void visit(const Map& M, Src& S, int tile, int round, int tx, int ty, int tz) {
  std::vector<double>& d = S.d;
  std::vector<uint8_t>&cur = S.flag[round & 1], &nxt = S.flag[(round + 1) & 1];
  static std::vector<double> st(gp::kStaged);
  cur[tile] = 0;
  S.rounds = round + 1;
  S.visits++;
  const int iz = tile % tz, iy = (tile / tz) % ty, ix = tile / (tz * ty);
  const int bx = ix * gp::kTile, by = iy * gp::kTile, bz = iz * gp::kTile;
  const double lim = S.bound;
  for (int hx = 0; hx < gp::kHalo; hx++)
    for (int hy = 0; hy < gp::kHalo; hy++)
      for (int hz = 0; hz < gp::kHalo; hz++) {
        const int x = bx + hx - 1, y = by + hy - 1, z = bz + hz - 1;
        st[gp::staged_index(hx, hy, hz)] = inside(M, x, y, z) ? d[x * M.YZ + y * M.Z + z] : gp::inf();
      }
  bool open[512];
  double pen[512];
  for (int t = 0; t < 256; t++)
    for (int j = 0; j < 2; j++) {
      const int lz = t & 7, lx = ((t >> 3) & 3) + 4 * j, ly = t >> 5, x = bx + lx, y = by + ly, z = bz + lz;
      const bool in = inside(M, x, y, z);
      const int gidx = in ? x * M.YZ + y * M.Z + z : 0;
      if (M.clear) {
        const int32_t dd = in ? M.d2[gidx] : 0;
        open[2 * t + j] = in && gp::clear_open(M.m[gidx], dd, M.min_d2);
        pen[2 * t + j] = open[2 * t + j] ? gp::clear_penalty(M.pen.data(), M.n_pen, dd) : 0.0;
      } else {
        open[2 * t + j] = in && M.m[gidx] == 0;
        pen[2 * t + j] = 0.0;
      }
    }
  int busy = 0;
  for (int it = 0; it < gp::kLocalIters; it++) {
    busy = 0;
    for (int t = 0; t < 256; t++)
      for (int j = 0; j < 2; j++) {
        if (!open[2 * t + j]) continue;
        const int lz = t & 7, lx = ((t >> 3) & 3) + 4 * j, ly = t >> 5;
        const int c = gp::staged_index(lx + 1, ly + 1, lz + 1);
        const double cand = M.clear ? gp::clear_candidate(st.data(), c, pen[2 * t + j]) : gp::relax_candidate(st.data(), c);
        if (gp::accept(cand, st[c], lim)) { st[c] = cand; busy = 1; }
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
      if (nx >= 0 && nx < tx && ny >= 0 && ny < ty && nz >= 0 && nz < tz) { nxt[(nx * ty + ny) * tz + nz] = 1; S.pending = round + 1; }
    }
}

struct Out { int rtn = 0, len = 0, min_d2 = 0x7fffffff; double cost = 0.0; std::vector<int> path, pd2; };

// k_fan_trace for one goal
static void trace(const Map& M, const int* s, const int* g, const std::vector<double>& d, int cap, Out& o) {
  int x = g[0], y = g[1], z = g[2];
  double dv = d[x * M.YZ + y * M.Z + z];
  o.cost = dv;
  if (!(dv < gp::inf())) { o.rtn = 1; return; }
  std::vector<int> back, bd2;
  for (;;) {
    const int v = x * M.YZ + y * M.Z + z;
    const int32_t dd = M.clear ? M.d2[v] : 0;
    back.push_back(x); back.push_back(y); back.push_back(z);
    bd2.push_back(dd);
    if (x == s[0] && y == s[1] && z == s[2]) break;
    if (M.clear && dd < o.min_d2) o.min_d2 = dd;
    const double pen = M.clear ? gp::clear_penalty(M.pen.data(), M.n_pen, dd) : 0.0;
    int k = 0;
    double du = 0.0;
    for (; k < 26; k++) {
      int dx, dy, dz;
      gp::neighbour(k, dx, dy, dz);
      du = inside(M, x + dx, y + dy, z + dz) ? d[(x + dx) * M.YZ + (y + dy) * M.Z + z + dz] : gp::inf();
      if (M.clear ? gp::clear_is_predecessor(du, k, pen, dv) : gp::is_predecessor(du, k, dv)) break;
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

// in: int32 X, Y, Z, n_src, n_goal, cap, max_rounds, fields, clear, min_d2, n_pen; uint8 map[G]; int32 d2[G]; float64 pen[n_pen];
//     int32 sources[n_src][3], goals[n_goal][3], goal_src[n_goal]
// out: per goal: int32 rtn, len, min_d2, 0; float64 cost; int32 path[n][3], d2[n], n = min(len, cap);
//      then per source: int32 stats[2]; float64 bound; float64 field[G] if fields
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[11];
  if (!f || fread(h, 4, 11, f) != 11) return 1;
  Map M;
  M.X = h[0]; M.Y = h[1]; M.Z = h[2]; M.YZ = M.Y * M.Z; M.G = M.X * M.YZ; M.clear = h[8]; M.min_d2 = h[9]; M.n_pen = h[10];
  Fan F;
  F.ns = h[3]; F.ng = h[4];
  const int cap = h[5], max_rounds = h[6], fields = h[7];
  M.m.resize(M.G); M.d2.resize(M.G); M.pen.resize(M.n_pen);
  F.src.resize(3 * F.ns); F.goal.resize(3 * F.ng); F.gsrc.resize(F.ng);
  if (fread(M.m.data(), 1, M.G, f) != (size_t)M.G || fread(M.d2.data(), 4, M.G, f) != (size_t)M.G ||
      fread(M.pen.data(), 8, M.n_pen, f) != (size_t)M.n_pen || fread(F.src.data(), 4, F.src.size(), f) != F.src.size() ||
      fread(F.goal.data(), 4, F.goal.size(), f) != F.goal.size() || fread(F.gsrc.data(), 4, F.gsrc.size(), f) != F.gsrc.size())
    return 1;
  fclose(f);
  // the host's grouping: a counting sort by source
  F.off.assign(F.ns + 1, 0);
  F.order.resize(F.ng);
  for (int j = 0; j < F.ng; j++) F.off[F.gsrc[j] + 1]++;
  for (int s = 0; s < F.ns; s++) F.off[s + 1] += F.off[s];
  {
    std::vector<int> at(F.off.begin(), F.off.end() - 1);
    for (int j = 0; j < F.ng; j++) F.order[at[F.gsrc[j]]++] = j;
  }
  const int tx = gp::tiles_along(M.X), ty = gp::tiles_along(M.Y), tz = gp::tiles_along(M.Z), nt = tx * ty * tz;
  std::vector<Src> S(F.ns);
  for (int s = 0; s < F.ns; s++) {  // k_path_init with ends = (source, source)
    const int* e = &F.src[3 * s];
    S[s].d.assign(M.G, gp::inf());
    S[s].flag[0].assign(nt, 0); S[s].flag[1].assign(nt, 0);
    if (!inside(M, e)) { S[s].pending = -1; continue; }
    S[s].d[e[0] * M.YZ + e[1] * M.Z + e[2]] = 0.0;
    S[s].flag[0][((e[0] / gp::kTile) * ty + e[1] / gp::kTile) * tz + e[2] / gp::kTile] = 1;
  }
  const long long lim = max_rounds > 0 ? max_rounds : gp::default_max_rounds(M.X, M.Y, M.Z);
  int done = 0;
  while (done < lim) {  // the host's batches of rounds, enqueued blindly, then one look at `pending`
    const int n = (int)(lim - done < gp::kFanRoundsPerCheck ? lim - done : gp::kFanRoundsPerCheck);
    for (int r = 0; r < n; r++) {
      if (r % FAN_BOUND_EVERY == 0)
        for (int s = 0; s < F.ns; s++) S[s].bound = bound_of(M, F, s, S[s].d);
      for (int s = 0; s < F.ns; s++)
        for (int tile = 0; tile < nt; tile++)
          if (S[s].flag[(done + r) & 1][tile]) visit(M, S[s], tile, done + r, tx, ty, tz);
    }
    done += n;
    bool live = false;
    for (int s = 0; s < F.ns; s++) live |= S[s].pending == done;
    if (!live) break;
  }
  FILE* o = fopen(argv[2], "wb");
  for (int j = 0; j < F.ng; j++) {
    const int s = F.gsrc[j];
    const int *e = &F.src[3 * s], *g = &F.goal[3 * j];
    Out r;
    if (!inside(M, e) || !inside(M, g)) { r.rtn = 2; r.cost = nan(""); }
    else if (S[s].pending == done) { r.rtn = 4; r.cost = nan(""); }
    else trace(M, e, g, S[s].d, cap, r);
    if (r.rtn == 1 || r.rtn == 2 || r.rtn == 4) r.min_d2 = 0x7fffffff;
    const int head[4] = {r.rtn, r.len, r.min_d2, 0};
    fwrite(head, 4, 4, o);
    fwrite(&r.cost, 8, 1, o);
    fwrite(r.path.data(), 4, r.path.size(), o);
    fwrite(r.pd2.data(), 4, r.pd2.size(), o);
  }
  for (int s = 0; s < F.ns; s++) {
    const int st[2] = {S[s].rounds, S[s].visits};
    fwrite(st, 4, 2, o);
    fwrite(&S[s].bound, 8, 1, o);
    if (fields) fwrite(S[s].d.data(), 8, M.G, o);
  }
  fclose(o);
  return 0;
}
'''


def build(workdir, local_iters=None, bound_every=1):
    """local_iters: sweeps per tile visit (DIRECT_GRIDPATH_LOCAL_ITERS; None: the library's); bound_every: 1 or 8, rounds between
    two refreshes of the bound"""
    assert bound_every in (1, 8)
    tag = "%s_%d" % ("lib" if local_iters is None else str(local_iters), bound_every)
    src = os.path.join(str(workdir), "grid_path_fan_harness.cpp")
    exe = os.path.join(str(workdir), "grid_path_fan_harness_" + tag)
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "direct_amd", "csrc"), src, "-o", exe, "-DFAN_BOUND_EVERY=%d" % bound_every]
                          + ([] if local_iters is None else ["-DDIRECT_GRIDPATH_LOCAL_ITERS=%d" % local_iters]))
    return str(workdir), exe


def is_clear(min_d2, penalty):
    return not (int(min_d2) <= 1 and (penalty is None or len(penalty) == 0))


def run(harness, grid, sources, goals, goal_src=None, d2=None, min_d2=0, penalty=None, path_capacity=4096, max_rounds=0, fields=True):
    """-> dict(rtn, path_len, path_cost, path_min_d2, paths: list of [n][3], path_d2: list of [n] (per goal); stats [S][2], bound [S],
    dist [S][G] or None (per source)).  Neutral mode (min_d2 <= 1, no table) needs no d2."""
    d, exe = harness
    grid = np.ascontiguousarray(grid, np.uint8)
    clear = is_clear(min_d2, penalty)
    d2 = np.zeros(grid.shape, np.int32) if d2 is None else np.ascontiguousarray(d2, np.int32)
    assert d2.shape == grid.shape
    pen = np.zeros(0) if penalty is None else np.ascontiguousarray(penalty, np.float64).reshape(-1)
    sources = np.ascontiguousarray(sources, np.int32).reshape(-1, 3)
    goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
    gs = np.zeros(len(goals), np.int32) if goal_src is None else np.ascontiguousarray(goal_src, np.int32).reshape(-1)
    S, n, G = len(sources), len(goals), grid.size
    assert len(gs) == n and (n == 0 or (gs.min() >= 0 and gs.max() < S))
    fin, fout = os.path.join(d, "fan_in.bin"), os.path.join(d, "fan_out.bin")
    with open(fin, "wb") as f:
        np.array(list(grid.shape) + [S, n, path_capacity, max_rounds, int(fields), int(clear), int(min_d2), len(pen)], np.int32).tofile(f)
        grid.tofile(f)
        d2.tofile(f)
        pen.tofile(f)
        sources.tofile(f)
        goals.tofile(f)
        gs.tofile(f)
    subprocess.check_call([exe, fin, fout])
    r = dict(rtn=np.zeros(n, np.int32), path_len=np.zeros(n, np.int32), path_cost=np.zeros(n), path_min_d2=np.zeros(n, np.int32), paths=[],
             path_d2=[], stats=np.zeros((S, 2), np.int32), bound=np.zeros(S), dist=np.zeros((S, G)) if fields else None)
    with open(fout, "rb") as f:
        for j in range(n):
            head = np.fromfile(f, np.int32, 4)
            r["rtn"][j], r["path_len"][j], r["path_min_d2"][j] = head[0], head[1], head[2]
            r["path_cost"][j] = np.fromfile(f, np.float64, 1)[0]
            k = min(int(head[1]), path_capacity)
            r["paths"].append(np.fromfile(f, np.int32, 3 * k).reshape(-1, 3))
            r["path_d2"].append(np.fromfile(f, np.int32, k))
        for s in range(S):
            r["stats"][s] = np.fromfile(f, np.int32, 2)
            r["bound"][s] = np.fromfile(f, np.float64, 1)[0]
            if fields:
                r["dist"][s] = np.fromfile(f, np.float64, G)
        assert f.read() == b""
    os.remove(fout)
    return r


def pairwise(ref_plain, ref_clear, grid, sources, goals, goal_src=None, d2=None, min_d2=0, penalty=None, path_capacity=4096):
    """every (sources[goal_src[j]], goals[j]) pair through the independent heap Dijkstra ("full") of the existing harnesses: the plain
    one in neutral mode, the clear one otherwise.  -> its dict, per goal, with dist [n][G] (the WHOLE component, exact)"""
    from tests import grid_path_clear_harness as gch
    sources = np.asarray(sources, np.int32).reshape(-1, 3)
    goals = np.asarray(goals, np.int32).reshape(-1, 3)
    gs = np.zeros(len(goals), np.int32) if goal_src is None else np.asarray(goal_src, np.int32)
    starts = sources[gs]
    if is_clear(min_d2, penalty):
        return gch.run(ref_clear, grid, d2, starts, goals, min_d2=min_d2, penalty=penalty, path_capacity=path_capacity, sides=("full",))["full"]
    return gh.run(ref_plain, grid, starts, goals, path_capacity=path_capacity, sides=("full",))["full"]


def same_per_goal(got, ref, clear, where=""):
    """the per-goal outputs of a fan result (host layout) against a pairwise result: codes, lengths, costs and paths to the bit"""
    n = len(ref["rtn"])
    assert np.array_equal(got["rtn"], ref["rtn"]), (where, got["rtn"], ref["rtn"])
    assert np.array_equal(got["path_len"], ref["path_len"]), where
    a, b = np.ascontiguousarray(got["path_cost"], np.float64), np.ascontiguousarray(ref["path_cost"], np.float64)
    assert ((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all(), (where, a, b)
    for j in range(n):
        assert np.array_equal(got["paths"][j], ref["paths"][j]), (where, j)
    if clear:
        assert np.array_equal(got["path_min_d2"], ref["path_min_d2"]), where
        for j in range(n):
            assert np.array_equal(got["path_d2"][j], ref["path_d2"][j]), (where, j)


def check_dist(got, ref, grid, sources, goals, goal_src, d2=None, min_d2=0, clear=False, where=""):
    """the dist contract per source: exact against the Dijkstra field wherever the true distance is <= the largest path_cost among the
    source's eligible goals (all of the component if one of them is unreachable), >= the true distance elsewhere.  ref: pairwise()'s
    result (its field of any goal of the source is the source's whole component).  -> per source the worst eligible cost (None
    without a goal inside the map)"""
    sources = np.asarray(sources).reshape(-1, 3)
    goals = np.asarray(goals).reshape(-1, 3)
    gs = np.zeros(len(goals), np.int32) if goal_src is None else np.asarray(goal_src)
    dims = np.array(grid.shape)
    worst = []
    for s in range(len(sources)):
        src = sources[s]
        if ((src < 0) | (src >= dims)).any():
            worst.append(None)
            continue
        mine = [j for j in range(len(goals)) if gs[j] == s and not ((goals[j] < 0) | (goals[j] >= dims)).any()]
        if not mine:
            worst.append(None)
            continue
        true = ref["dist"][mine[0]]
        lim = 0.0
        for j in mine:
            g = tuple(goals[j])
            ok = (goals[j] == src).all() or (grid[g] == 0 and (not clear or d2[g] >= min_d2))
            if ok:
                lim = max(lim, true[np.ravel_multi_index(g, grid.shape)])
        worst.append(lim)
        mine_d = got["dist"][s]
        sel = true <= lim
        assert np.array_equal(mine_d[sel].view(np.int64), true[sel].view(np.int64)), (where, s)
        assert (mine_d >= true).all(), (where, s)
    return worst


def regroup_by_start(starts, goals):
    """(start, goal) pairs -> sources (the distinct starts, in order of first appearance), goals, goal_src"""
    starts = np.asarray(starts, np.int32).reshape(-1, 3)
    keys, sources, gs = {}, [], []
    for s in starts:
        k = tuple(int(v) for v in s)
        if k not in keys:
            keys[k] = len(sources)
            sources.append(k)
        gs.append(keys[k])
    return np.array(sources, np.int32), np.asarray(goals, np.int32).reshape(-1, 3), np.array(gs, np.int32)
