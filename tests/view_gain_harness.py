"""Visible unknown volume per candidate viewpoint (include/direct_cluster.h, "visible unknown volume per candidate viewpoint") -
TEST INFRASTRUCTURE of tests/test_view_gain_restatement.py, tests/test_gpu_view_gain.py and tools/view_gain_bench.py.  Two sides:
  restate       an independent restatement in Python floats (which are C doubles, with no fused multiply-add), written from the
                definition's TEXT and not from direct_amd/csrc/view_gain_math.h: one ray loop and a Python set per candidate.
  build / run   view_gain_math.h compiled by g++ into ONE stand-alone program with its own main that emulates the workgroup of
                k_view_gain as a lane loop on one thread, with the box of bits and its first-setter rule; it also times itself,
                for the bench tool.  build(..., sanitize=True) is the same program under -fsanitize=address,undefined.
and the scenes, candidates and direction sets the CPU and GPU tests share.  There is no reference counterpart."""
import functools
import math
import os
import subprocess

import numpy as np

from tests import free_comp_harness as fh
from tests import map_scan_harness as sh
from tests.cpp_program import compile_program

ROOT = sh.ROOT
OK, OUTSIDE, OCCUPIED, BAD_SET = 0, 1, 2, 3
BLOCKED, LEFT, RANGE, SKIPPED = 0, 1, 2, 3
KEYS = ("code", "gain", "seen", "ends")
MAX_R = 50


def box_half(range_vox):
    return int(math.floor(range_vox)) + 2


# ---- the restatement -------------------------------------------------------------------------------------------------------
def ray(grid, v0, d, range_vox):
    """One ray from the centre of v0 (inside the map).  -> (outcome, the voxels visited, in order)"""
    d = [float(d[0]), float(d[1]), float(d[2])]
    if not all(math.isfinite(v) for v in d):
        return SKIPPED, []
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    if dd == 0.0:
        return SKIPPED, []
    R2 = float(range_vox) * float(range_vox)
    dims = grid.shape
    i = [int(v0[0]), int(v0[1]), int(v0[2])]
    step = [(v > 0.0) - (v < 0.0) for v in d]
    tdel = [1.0 / abs(d[a]) if step[a] else None for a in range(3)]
    tmax = [0.5 * tdel[a] if step[a] else None for a in range(3)]
    axes = [a for a in range(3) if step[a]]
    visited = []
    for _ in range(3 * box_half(range_vox) + 3):
        if not (0 <= i[0] < dims[0] and 0 <= i[1] < dims[1] and 0 <= i[2] < dims[2]):
            return LEFT, visited
        visited.append((i[0], i[1], i[2]))
        if grid[i[0], i[1], i[2]] != 0:
            return BLOCKED, visited
        c = axes[0]
        for a in axes[1:]:
            if tmax[a] < tmax[c]:
                c = a
        t = tmax[c]
        if not ((t * t) * dd <= R2):
            return RANGE, visited
        i[c] += step[c]
        tmax[c] += tdel[c]
    raise AssertionError("the walk passed its trip bound")


def restate(grid, known, voxels, dirs, range_vox, sets=None):
    """-> dict(code, gain, seen [n], ends [n][4], visited: the set of voxels per candidate, max_offset [n]: the largest per-axis
    offset from the candidate among them, -1 without one)"""
    grid, known = np.asarray(grid), np.asarray(known)
    vox = np.asarray(voxels, np.int64).reshape(-1, 3)
    d = np.asarray(dirs, np.float32)
    d = d.reshape((1,) + d.shape) if d.ndim == 2 else d
    n = len(vox)
    out = dict(code=np.zeros(n, np.int32), gain=np.zeros(n, np.int32), seen=np.zeros(n, np.int32), ends=np.zeros((n, 4), np.int32),
               visited=[set() for _ in range(n)], max_offset=np.full(n, -1, np.int32))
    for c in range(n):
        v0, s = tuple(int(v) for v in vox[c]), 0 if sets is None else int(sets[c])
        if not all(0 <= v0[a] < grid.shape[a] for a in range(3)):
            out["code"][c] = OUTSIDE
        elif grid[v0] != 0:
            out["code"][c] = OCCUPIED
        elif not 0 <= s < len(d):
            out["code"][c] = BAD_SET
        if out["code"][c] != OK:
            continue
        seen = out["visited"][c]
        for row in d[s]:
            end, visited = ray(grid, v0, row, range_vox)
            out["ends"][c, end] += 1
            seen.update(visited)
        out["seen"][c] = len(seen)
        out["gain"][c] = sum(1 for v in seen if known[v] == 0)
        out["max_offset"][c] = max((max(abs(v[a] - v0[a]) for a in range(3)) for v in seen), default=-1)
    return out


def assert_same(got, want, what=""):
    for k in KEYS:
        g = got[k]
        g = np.asarray(g.cpu() if hasattr(g, "cpu") else g)
        assert g.dtype == np.int32 and g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k, g, want[k])


# ---- scenes, candidates and direction sets the CPU and GPU tests share ---------------------------------------------------------
DYADIC = dict(dims=(32, 32, 16), res=0.25, lower=np.array([-4.0, -4.0, 0.0]), upper=np.array([4.0, 4.0, 4.0]), v0=(13, 17, 6))
DYADIC_RANGES = (0.7, 1.5, 2.25, 10.0)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (map, known): 20 % random occupancy with 50 % random known and the empty map with nothing / everything known on
    fh.DIMS; the map and the known grid two tracked scans of sh.wall_and_room() leave on sh.DIMS"""
    rng = np.random.default_rng(41)
    out = dict(random=((rng.random(fh.DIMS) < 0.2).astype(np.uint8), (rng.random(fh.DIMS) < 0.5).astype(np.uint8)),
               empty_unknown=(np.zeros(fh.DIMS, np.uint8), np.zeros(fh.DIMS, np.uint8)),
               empty_known=(np.zeros(fh.DIMS, np.uint8), np.ones(fh.DIMS, np.uint8)))
    from tests import frontier_harness as fr
    wpts, room, _ = sh.wall_and_room()
    raw, _, _ = sh.restate(wpts, sh.ORIGIN, 10.0)
    _, grid, _ = sh.restate(room, sh.ORIGIN, 10.0, raw=raw)
    known = fr.known_restate(room, sh.ORIGIN, 10.0, known=fr.known_restate(wpts, sh.ORIGIN, 10.0))
    out["wall_and_room"] = (grid, known)
    return out


def candidates(grid, n_free=6, seed=9):
    """[k][3] int32: the eight corners' first and last, a face, an edge, voxels outside the map on every side and far away, the
    first occupied voxels, then n_free random free voxels.  With an occupied corner the corner candidate is an occupied one."""
    X, Y, Z = grid.shape
    fixed = [(0, 0, 0), (X - 1, Y - 1, Z - 1), (X // 2, 0, Z // 2), (0, Y - 1, Z // 3), (-1, 2, 2), (2, Y, 2), (2, 2, -1), (X, Y, Z),
             (-2 ** 31, 0, 0), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]
    occ = np.argwhere(grid != 0)[:2].tolist()
    free = np.argwhere(grid == 0)
    pick = free[np.random.default_rng(seed).choice(len(free), min(n_free, len(free)), replace=False)].tolist()
    return np.array(fixed + occ + pick, np.int64).astype(np.int32).reshape(-1, 3)


def dirs_sign():
    """the 26 sign directions: exact tmax ties between two and three axes at every step"""
    return np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float32)


def dirs_axis():
    return np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)


def dirs_random(n, seed=7):
    """normal directions of any length; some far from 1"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)) * np.exp(rng.uniform(-3, 3, (n, 1)))
    return d.astype(np.float32)


def dirs_degenerate():
    """NaN, infinity and zero rows (skipped), signed zeros and a denormal beside good components (not skipped)"""
    nan, inf, tiny = float("nan"), float("inf"), 1e-42
    return np.array([(nan, 1, 0), (0, -inf, 1), (1, 2, nan), (inf, inf, inf), (0, 0, 0), (-0.0, 0.0, -0.0), (-0.0, 1, 0), (0, -0.0, -3),
                     (tiny, 0, 0), (tiny, -tiny, tiny), (1, 1, 1), (nan, nan, nan), (2, -0.5, 0.25)], np.float32)


def dirs_dyadic(n=300, seed=3):
    """n distinct nonzero directions with components k / 8, |k| <= 8: every quantity of the walk scales by a power of two between
    voxel units and a grid of resolution 0.25"""
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(-8, 9, (4 * n, 3)), axis=0)
    k = k[np.any(k != 0, axis=1)]
    k = k[rng.permutation(len(k))[:n]]
    assert len(k) == n
    return (k / 8.0).astype(np.float32)


def dyadic_cloud(dirs):
    """the points centre + 64 * dir of the dyadic grid's candidate, exact in float32, and the centre"""
    centre = DYADIC["lower"] + (np.array(DYADIC["v0"]) + 0.5) * DYADIC["res"]
    pts = centre + 64.0 * np.asarray(dirs, np.float64)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    return pts.astype(np.float32), centre


# ---- the header, compiled by g++ -----------------------------------------------------------------------------------------------
HARNESS = r'''
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "view_gain_math.h"
namespace vg = direct::viewgain;

template <typename T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
template <typename T> static void wr(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

// in: int32 X, Y, Z, n, n_dirs, n_sets, has_set, lanes, reps; float64 range_vox; int32 voxel[n][3]; int32 set[n] when has_set;
//     float32 dirs[n_sets][n_dirs][3]; uint8 map[G], known[G]
// out: int32 err (the error word); float64 ms (best of reps); int32 code[n], gain[n], seen[n], ends[n][4], max_offset[n];
//      int64 visits (voxels visited by all rays, repeats included)
// Exit status 3: the range is not supported
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 1;
  const std::vector<int32_t> h = rd<int32_t>(fi, 9);
  const double range_vox = rd<double>(fi, 1)[0];
  const int n = h[3], n_dirs = h[4], n_sets = h[5], has_set = h[6], lanes = h[7], reps = h[8];
  const size_t G = (size_t)h[0] * h[1] * h[2];
  const std::vector<int32_t> voxel = rd<int32_t>(fi, 3 * (size_t)n), set = rd<int32_t>(fi, has_set ? n : 0);
  const std::vector<float> dirs = rd<float>(fi, (size_t)n_sets * n_dirs * 3);
  const std::vector<uint8_t> map = rd<uint8_t>(fi, G), known = rd<uint8_t>(fi, G);
  fclose(fi);
  if (!(range_vox > 0.0) || !vg::supported(range_vox)) return 3;
  vg::Scene S;
  S.size[0] = h[0]; S.size[1] = h[1]; S.size[2] = h[2];
  S.R = vg::box_half(range_vox);
  S.R2 = range_vox * range_vox;
  std::vector<uint32_t> bits(vg::box_words(S.R));
  std::vector<int32_t> code(n), gain(n), seen(n), ends(4 * (size_t)n), max_offset(n);
  int32_t err = 0;
  int64_t visits = 0;
  double best = 1e300;
  for (int rep = 0; rep < reps; rep++) {
    visits = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int c = 0; c < n; c++) {  // one workgroup of k_view_gain
      const int* v0 = &voxel[3 * (size_t)c];
      const int s = has_set ? set[c] : 0;
      code[c] = vg::candidate_code(S, map.data(), v0, s, n_sets);
      gain[c] = seen[c] = 0;
      max_offset[c] = -1;
      for (int k = 0; k < 4; k++) ends[4 * (size_t)c + k] = 0;
      if (code[c] != vg::kOk) continue;
      std::fill(bits.begin(), bits.end(), 0u);
      const float* set_dirs = &dirs[(size_t)s * n_dirs * 3];
      for (int lane = 0; lane < lanes; lane++)      // the lanes one after the other
        for (int r = lane; r < n_dirs; r += lanes) {
          const float* q = set_dirs + 3 * (size_t)r;
          const int end = vg::cast_ray(S, map.data(), v0, q[0], q[1], q[2], [&](const int* i, size_t at) {
            const int bit = vg::box_bit(S.R, v0, i);
            if (bit < 0) { err |= vg::kErrBox; return; }
            visits++;
            const uint32_t m = 1u << (bit & 31);
            const uint32_t old = bits[bit >> 5];   // the returning atomic OR
            bits[bit >> 5] = old | m;
            if (old & m) return;
            seen[c]++;
            gain[c] += known[at] == 0;
            for (int a = 0; a < 3; a++) {
              const int o = i[a] > v0[a] ? i[a] - v0[a] : v0[a] - i[a];
              if (o > max_offset[c]) max_offset[c] = o;
            }
          });
          if (end < 0) err |= vg::kErrTrips;
          else ends[4 * (size_t)c + end]++;
        }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms < best) best = ms;
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 1;
  fwrite(&err, 4, 1, fo);
  fwrite(&best, 8, 1, fo);
  wr(fo, code); wr(fo, gain); wr(fo, seen); wr(fo, ends); wr(fo, max_offset);
  fwrite(&visits, 8, 1, fo);
  fclose(fo);
  return 0;
}
'''


def build(workdir, sanitize=False):
    name = "view_gain_harness_san" if sanitize else "view_gain_harness"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    return compile_program(workdir, name, HARNESS, extra)


def run(exe, grid, known, voxels, dirs, range_vox, sets=None, lanes=256, reps=1):
    """-> dict(code, gain, seen, ends, max_offset, ms, visits) of the header program; its error word must be 0"""
    grid = np.ascontiguousarray(grid, np.uint8)
    vox = np.ascontiguousarray(voxels, np.int32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32)
    d = d.reshape((1,) + d.shape) if d.ndim == 2 else d
    n = len(vox)
    fin, fout = exe + ".in", exe + ".out"
    with open(fin, "wb") as f:
        np.array(list(grid.shape) + [n, d.shape[1], d.shape[0], int(sets is not None), lanes, reps], np.int32).tofile(f)
        np.array([range_vox], np.float64).tofile(f)
        vox.tofile(f)
        if sets is not None:
            np.ascontiguousarray(sets, np.int32).tofile(f)
        d.tofile(f)
        grid.tofile(f)
        np.ascontiguousarray(known, np.uint8).tofile(f)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    with open(fout, "rb") as f:
        err = int(np.fromfile(f, np.int32, 1)[0])
        ms = float(np.fromfile(f, np.float64, 1)[0])
        out = dict(code=np.fromfile(f, np.int32, n), gain=np.fromfile(f, np.int32, n), seen=np.fromfile(f, np.int32, n),
                   ends=np.fromfile(f, np.int32, 4 * n).reshape(n, 4), max_offset=np.fromfile(f, np.int32, n), ms=ms)
        out["visits"] = int(np.fromfile(f, np.int64, 1)[0])
        assert f.read() == b""
    os.remove(fin)
    os.remove(fout)
    assert err == 0, "a walk left its box or passed its trip bound (error word %d)" % err
    return out
