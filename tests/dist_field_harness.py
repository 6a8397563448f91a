"""TEST INFRASTRUCTURE of tests/test_dist_field_cpp.py, tests/test_plan_clear_restatement.py, tests/test_gpu_dist_field.py,
tests/test_gpu_plan_clear.py and tools/dist_field_bench.py: what direct_cluster_distance_field and
direct_cluster_plan_clearance_batch (include/direct_cluster.h) must return, twice over.
  brute_d2            NumPy, written from the header's text, NOT from direct_amd/csrc/dist_field_math.h: the minimum over ALL
                      occupied voxels of the squared distance, pair by pair.  Where the pairs are too many for a quick test
                      (over PAIR_LIMIT) the same minimum is taken axis by axis over whole lines (every j of every line, no
                      early exit, no envelope); the CPU test checks the two against each other wherever both can run.
  restate_clearance   NumPy, written from the header's text, NOT from plan_clear_math.h: it forms ALL 2^D leaves of every segment
                      with plan_check_harness.halve_all and evaluates every one of them.
  build / run_field / run_clear   a g++ -O2 -ffp-contract=off program around dist_field_math.h and plan_clear_math.h that runs
                      the headers on one thread (and times the field, for the bench tool).
  cube_distance       exact distance of points to the union of occupied voxel CUBES, point by point and cube by cube: the
                      soundness test's yardstick, independent of both implementations.
and the grids the CPU and the GPU tests share."""
import os
import subprocess

import numpy as np

from tests import plan_check_harness as ph
from tests.cpp_program import compile_program
from tests.map_cloud_harness import LOWER, RES

ROOT = ph.ROOT
NONE = 0x7fffffff
K = float.fromhex("0x1.bb67ae8584cabp-1")
PAIR_LIMIT = 2e8
INVALID = -1


# ---- the field ---------------------------------------------------------------------------------------------------------

def cap2_of(cap_vox):
    return cap_vox * cap_vox if cap_vox > 0 else NONE


def _pairwise(grid):
    occ = np.argwhere(grid == 1).astype(np.int64)
    vox = np.argwhere(np.ones(grid.shape, bool)).astype(np.int64)
    out = np.full(len(vox), NONE, np.int64)
    if len(occ):
        step = max(1, int(4e6) // len(occ))
        for s in range(0, len(vox), step):
            d = vox[s:s + step, None, :] - occ[None, :, :]
            out[s:s + step] = (d * d).sum(axis=2).min(axis=1)
    return out.reshape(grid.shape)


def _linewise(grid):
    """the same minimum, axis by axis over whole lines: min_ux ((vx-ux)^2 + min_uy ((vy-uy)^2 + min_uz (vz-uz)^2))"""
    INF = np.int64(1) << 40
    f = np.where(grid == 1, 0, INF).astype(np.int64)
    for axis in (2, 1, 0):
        n = grid.shape[axis]
        k = np.arange(n, dtype=np.int64)
        cost = (k[:, None] - k[None, :]) ** 2                 # [i][j]
        g = np.moveaxis(f, axis, -1)                          # [...][j]
        f = np.moveaxis((g[..., None, :] + cost).min(axis=-1), -1, axis)
    return np.where(f >= INF, NONE, f)


def brute_d2(grid, cap_vox=0, force=None):
    """-> int32 [X][Y][Z], the stored field of the header's definition"""
    grid = np.asarray(grid, np.uint8)
    pairs = float(np.count_nonzero(grid == 1)) * grid.size
    how = force or ("pairwise" if pairs <= PAIR_LIMIT else "linewise")
    d2 = _pairwise(grid) if how == "pairwise" else _linewise(grid)
    return np.minimum(d2, cap2_of(cap_vox)).astype(np.int32)


def field_stats(d2, cap_vox):
    below = d2[d2 < cap2_of(cap_vox)]
    return dict(below_cap=int(below.size), max_d2=int(below.max()) if below.size else -1)


SHAPES = ((1, 1, 1), (67, 5, 3), (3, 130, 2), (2, 3, 261), (65, 64, 63))
DENSITIES = ("empty", "corner", "1%", "30%", "100%")
CAPS = (0, 1, 4)


def random_grid(shape, density, seed=0):
    rng = np.random.default_rng(seed + 7 * DENSITIES.index(density) + sum(shape))
    g = np.zeros(shape, np.uint8)
    if density == "corner":
        g[-1, 0, -1] = 1
    elif density == "100%":
        g[:] = 1
    elif density != "empty":
        g = (rng.random(shape) < float(density[:-1]) / 100.0).astype(np.uint8)
    return g


def shared_grids():
    """-> list of (name, grid): the plan check's map, then every shape at every density"""
    out = [("shared_map", ph.shared_map())]
    for shape in SHAPES:
        for density in DENSITIES:
            out.append(("%dx%dx%d %s" % (shape + (density,)), random_grid(shape, density)))
    return out


# ---- the clearance -----------------------------------------------------------------------------------------------------

def leaf_bounds(L, d2, lower, res):
    """[n][3][6] leaves -> (bound [n], half [n], centre inside the map [n])"""
    size = np.asarray(d2.shape, np.float64)
    inv = 1.0 / res
    with np.errstate(all="ignore"):
        lo, hi = L.min(axis=2), L.max(axis=2)
        c = (lo + hi) * 0.5
        e = (hi - lo) * 0.5
        half = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        q = (c - lower) * inv
        mid = np.trunc(np.where((q >= 1) & (q < size), q, 0.0)).astype(np.int64)
        idx = np.where(q >= size, np.asarray(d2.shape) - 1, np.where(~(q >= 1), 0, mid))
        m = (idx.astype(np.float64) + 0.5) * res + lower
        r = c - m
        off = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        v = d2[idx[:, 0], idx[:, 1], idx[:, 2]]
        bound = ((np.sqrt(np.where(v == NONE, 0, v).astype(np.float64)) - K) * res - off) - half
        bound = np.where(v == NONE, np.inf, bound)
        inside = ((q >= 0) & (q < size)).all(axis=1)
    return bound, half, inside


def restate_clearance(inp, d2, depth, radius=0.0, use_t_from=True, lower=LOWER, res=RES):
    """inp as plan_check_harness.plan_rows takes it; d2: the stored field -> dict of the call's outputs as they read in HOST memory,
    plus half_max [B] (the largest leaf half-diagonal of the row) and centre_inside [B] (of the minimising leaf's box)"""
    T, t_from, rows = ph.plan_rows(inp, use_t_from)
    B, N = T.shape
    lower = np.asarray(lower, np.float64)
    nan_fill = np.frombuffer(b"\xff" * 8, np.float64)[0]
    out = dict(status=np.zeros(B, np.int32), clearance=np.zeros(B), where=np.full((B, 2), -1, np.int32), t_min=np.zeros(B),
               verdict=np.zeros(B, np.int32), t_free=np.zeros(B), seg_clearance=np.full((B, N), nan_fill),
               half_max=np.zeros(B), centre_inside=np.zeros(B, bool))
    for b, (n, ok, pts, S) in enumerate(rows):
        if not ok:
            out["status"][b], out["verdict"][b], out["clearance"][b] = -1, INVALID, np.nan
            out["seg_clearance"][b, :max(0, min(n, N))] = np.nan
            continue
        out["t_min"][b] = out["t_free"][b] = S[n]
        best, free_found = np.inf, False
        for i in range(n):
            L = ph.leaves(pts[i], depth)
            k = np.arange(1 << depth, dtype=np.float64)
            t0 = S[i] + (k * 2.0 ** -depth) * T[b, i]
            t1 = S[i] + ((k + 1) * 2.0 ** -depth) * T[b, i]
            judged = np.ones(len(k), bool) if t_from is None else t1 > t_from[b]
            bound, half, inside = leaf_bounds(L, d2, lower, res)
            out["half_max"][b] = max(out["half_max"][b], half.max())
            jb = np.where(judged, bound, np.inf)
            kk = int(np.argmin(jb))
            out["seg_clearance"][b, i] = jb[kk]
            if jb[kk] < best:
                best = jb[kk]
                out["where"][b] = (i, kk)
                out["t_min"][b] = t0[kk]
                out["centre_inside"][b] = inside[kk]
            below = judged & (bound < radius)
            if below.any() and not free_found:
                free_found = True
                out["verdict"][b], out["t_free"][b] = 1, t0[int(np.argmax(below))]
        out["clearance"][b] = best
    return out


def cube_distance(points, grid, lower=LOWER, res=RES):
    """exact distance [m] of every point to the union of the occupied voxels' closed cubes (+inf on an empty map)"""
    occ = np.argwhere(grid == 1).astype(np.float64)
    points = np.asarray(points, np.float64)
    out = np.full(len(points), np.inf)
    if not len(occ):
        return out
    clo = np.asarray(lower) + occ * res
    chi = clo + res
    step = max(1, int(2e6) // len(occ))
    for s in range(0, len(points), step):
        p = points[s:s + step, None, :]
        d = np.maximum(np.maximum(clo[None] - p, p - chi[None]), 0.0)
        out[s:s + step] = np.sqrt((d * d).sum(axis=2)).min(axis=1)
    return out


# ---- the headers, compiled by g++ --------------------------------------------------------------------------------------

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dist_field_math.h"
#include "plan_clear_math.h"
''' + ph.ROW_FRONT + r'''
namespace dfm = direct::distfield;
namespace pc = direct::planclear;
// field  in: int32 X, Y, Z, cap_vox, reps, pad; uint8 map[G]            out: int32 d2[G]; int64 stats[2]; float64 ms (best of reps)
// clear  in: int32 B, N, poly, D, has_from, X, Y, Z; float64 lower[3], res, radius; the row section; int32 d2[G]
//        out: int32 status[B], verdict[B], where[B][2]; float64 clearance[B], t_min[B], t_free[B], seg_clearance[B][N]
static int field(FILE* f, const char* to) {
  int h[6];
  if (fread(h, 4, 6, f) != 6) return 1;
  const int X = h[0], Y = h[1], Z = h[2], cap = h[3], reps = h[4];
  const size_t G = (size_t)X * Y * Z;
  std::vector<uint8_t> map(G);
  if (fread(map.data(), 1, G, f) != G) return 1;
  std::vector<int32_t> d2(G), tmp(G);
  double best = 1e300;
  for (int rep = 0; rep < reps; rep++) {
    const auto c0 = std::chrono::steady_clock::now();
    dfm::field_host(map.data(), X, Y, Z, cap, d2.data(), tmp.data());
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    if (ms < best) best = ms;
  }
  int64_t stats[2];
  dfm::stats_host(d2.data(), (long long)G, cap, stats);
  FILE* o = fopen(to, "wb");
  if (!o) return 1;
  fwrite(d2.data(), 4, G, o);
  fwrite(stats, 8, 2, o);
  fwrite(&best, 8, 1, o);
  fclose(o);
  return 0;
}
static int clear(FILE* f, const char* to) {
  int h[8];
  double d[5];
  if (fread(h, 4, 8, f) != 8 || fread(d, 8, 5, f) != 5) return 1;
  const int B = h[0], N = h[1], D = h[3], has_from = h[4], X = h[5], Y = h[6], Z = h[7];
  const size_t G = (size_t)X * Y * Z;
  Rows R = {B, N, h[2], has_from};
  std::vector<int32_t> d2(G);
  if (!read_rows(f, R) || fread(d2.data(), 4, G, f) != G) return 1;
  pc::Grid grid;
  grid_front(grid, d, d[3], X, Y, Z);
  grid.resolution = d[3];
  const double radius = d[4];
  auto d2_at = [&](int i0, int i1, int i2) { return d2[((size_t)i0 * Y + i1) * Z + i2]; };
  std::vector<int> status(B), verdict(B), where((size_t)B * 2, -1);
  std::vector<double> clearance(B), t_min(B), t_free(B), seg((size_t)B * N), S(N + 1), P;
  memset(seg.data(), 0xff, seg.size() * 8);
  const double nan = __builtin_nan("");
  const int dl = D < 6 ? D : 6;
  for (int b = 0; b < B; b++) {
    const int n = R.n_seg[b], ok = row_front(R, b, S, P);
    status[b] = ok ? 0 : -1;
    verdict[b] = ok ? 0 : -1;
    clearance[b] = ok ? (double)INFINITY : nan;
    t_min[b] = t_free[b] = ok ? S[n] : 0.0;
    if (!ok) {
      for (int i = 0; i < (n < 0 ? 0 : (n > N ? N : n)); i++) seg[(size_t)b * N + i] = nan;
      continue;
    }
    for (int i = 0; i < n; i++) {
      const double Ti = R.T[(size_t)b * N + i];
      // the kernels' split into subtrees of depth min(D, 6), merged in DESCENDING order: the merge must not care
      pc::SegMin r = {(double)INFINITY, pc::kNoLeaf, pc::kNoLeaf};
      for (int l = (1 << dl) - 1; l >= 0; l--)
        r = pc::merge(r, pc::subtree_min(&P[i * 18], S[i], Ti, D, dl, l, has_from, R.t_from[b], radius, grid, d2_at));
      seg[(size_t)b * N + i] = r.best;
      if (r.best < clearance[b]) {
        clearance[b] = r.best;
        where[b * 2] = i; where[b * 2 + 1] = r.leaf;
        t_min[b] = pk::node_time(S[i], Ti, D, r.leaf);
      }
      if (r.below != pc::kNoLeaf && verdict[b] == 0) {
        verdict[b] = 1;
        t_free[b] = pk::node_time(S[i], Ti, D, r.below);
      }
    }
  }
  FILE* o = fopen(to, "wb");
  if (!o) return 1;
  fwrite(status.data(), 4, B, o);
  fwrite(verdict.data(), 4, B, o);
  fwrite(where.data(), 4, where.size(), o);
  fwrite(clearance.data(), 8, B, o);
  fwrite(t_min.data(), 8, B, o);
  fwrite(t_free.data(), 8, B, o);
  fwrite(seg.data(), 8, seg.size(), o);
  fclose(o);
  return 0;
}
int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 1;
  const int rc = argv[1][0] == 'f' ? field(f, argv[3]) : clear(f, argv[3]);
  fclose(f);
  return rc;
}
'''


def build(workdir):
    return str(workdir), compile_program(workdir, "dist_field_harness", HARNESS)


def run_field(harness, grid, cap_vox=0, reps=1):
    """-> (d2 int32 [X][Y][Z], stats dict, ms) of dist_field_math.h on one thread"""
    d, exe = harness
    fin, fout = os.path.join(d, "field_in.bin"), os.path.join(d, "field_out.bin")
    with open(fin, "wb") as f:
        np.array(list(grid.shape) + [cap_vox, reps, 0], np.int32).tofile(f)
        np.ascontiguousarray(grid, np.uint8).tofile(f)
    subprocess.check_call([exe, "field", fin, fout])
    with open(fout, "rb") as f:
        d2 = np.fromfile(f, np.int32, grid.size).reshape(grid.shape)
        stats = np.fromfile(f, np.int64, 2)
        ms = float(np.fromfile(f, np.float64, 1)[0])
        assert f.read() == b""
    os.remove(fout)
    return d2, dict(below_cap=int(stats[0]), max_d2=int(stats[1])), ms


def run_clear(harness, inp, d2, depth, radius=0.0, use_t_from=True, lower=LOWER, res=RES):
    """-> outputs as restate_clearance gives them (without half_max / centre_inside) of plan_clear_math.h on one thread"""
    d, exe = harness
    (B, N, poly, has_from), rows = ph.row_section(inp, use_t_from)
    fin, fout = os.path.join(d, "clear_in.bin"), os.path.join(d, "clear_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([B, N, poly, depth, has_from] + list(d2.shape), np.int32).tobytes())
        f.write(np.array(list(lower) + [res, radius], np.float64).tobytes() + rows + np.ascontiguousarray(d2, np.int32).tobytes())
    subprocess.check_call([exe, "clear", fin, fout])
    with open(fout, "rb") as f:
        out = dict(status=np.fromfile(f, np.int32, B), verdict=np.fromfile(f, np.int32, B), where=np.fromfile(f, np.int32, B * 2).reshape(B, 2),
                   clearance=np.fromfile(f, np.float64, B), t_min=np.fromfile(f, np.float64, B), t_free=np.fromfile(f, np.float64, B),
                   seg_clearance=np.fromfile(f, np.float64, B * N).reshape(B, N))
        assert f.read() == b""
    os.remove(fout)
    return out


KEYS = ("status", "verdict", "where", "clearance", "t_min", "t_free", "seg_clearance")


def assert_same(got, want, what=""):
    """every integer and every bit of the doubles; a NaN (an invalid row's, or the fill past n_seg) must meet a NaN, whatever
    its payload"""
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, f"{what}: {k} has shape {g.shape}, not {w.shape}"
        if g.dtype.kind == "f":
            gn, wn = np.isnan(g), np.isnan(w)
            same = np.array_equal(gn, wn) and np.array_equal(g[~gn].view(np.uint64), w[~wn].view(np.uint64))
        else:
            same = np.array_equal(g, w)
        assert same, f"{what}: {k} differs\n{got[k]}\n{want[k]}"


# ---- inputs ------------------------------------------------------------------------------------------------------------

def leaving_row():
    """one plan that starts inside the map, leaves it through the lower x face and ends 4 m outside: box centres outside the map"""
    y, z = ph.lane_y(6), ph.LANE_Z
    rows = [[(ph._line([-2.5, y, z], [-3.4, y, z]), 1.0), (ph._line([-3.4, y, z], [-7.0, y + 0.5, z + 3.0]), 1.5)]]
    return ph.pack(rows, 2, np.array([0.25]))


def clear_inputs():
    """plan_check_harness.shared_inputs() plus the row that leaves the map"""
    out = ph.shared_inputs()
    out["leaving1"] = leaving_row()
    return out


# every listed value of every option appears: (kind, float32 storage, use t_from, radius)
COMBOS = (("bez", False, True, 0.0), ("poly", True, False, 0.3), ("bez", True, True, 0.3), ("poly", False, False, 0.0))
