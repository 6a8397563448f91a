"""TEST INFRASTRUCTURE of tests/test_map_cloud_restatement.py, tests/test_gpu_map_cloud.py and tools/map_cloud_bench.py: what the
map of direct_cluster_map_from_cloud (include/direct_cluster.h) must be, three times over.
  restate      NumPy, written from the reference's text (rcvPointCloudCallBack, global_planner/src/teach_repeat_planner.cpp:523-581,
               with utils/a_star.h:141-149 and utils/a_star.cpp:74-85), NOT from direct_amd/csrc/map_cloud_math.h: per axis the
               list of indices of the shifted coordinates, the map as their Cartesian product.  Both border conventions.
  triple_loop  the reference's loop nest, literally, in Python: for small inputs.
  build / run  a g++ -O2 program around map_cloud_math.h that runs the reference's loop nest on one thread with the HEADER's
               functions (the pattern of tests/grid_path_harness.py); it also times itself, for the bench tool.
Where the reference is undefined the three follow the contract of the C-ABI: a point with a non-finite coordinate contributes
nothing; under "drop" an index >= size is dropped like a coordinate >= upper."""
import math
import os
import subprocess

import numpy as np

from tests.cpp_program import compile_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLAMP, DROP = 0, 1

# the map of the issue's CPU experiment; the upper corner in z lies 0.05 above 12 voxels, as the launch file's 5.0 m lies above
# 33 voxels of 0.15 m: coordinates in that gap pass setObs' range test and index one past the array in the reference
DIMS, RES, LOWER, UPPER = (40, 36, 12), 0.15, np.array([-3.0, -2.7, 0.0]), np.array([3.0, 2.7, 1.85])
MARGINS = (0.0, 0.25, 0.45)


def steps(margin, res):
    """TRP:537-538: C's round() is half away from zero, the margin is not negative"""
    s = int(math.floor(margin * (1.0 / res) + 0.5))
    return s, max(1, s // 2)


def _rows(points):
    """float32 [n][3 or 4]; an empty cloud has no second dimension to infer"""
    pts = np.asarray(points, np.float32)
    return pts.reshape(len(pts), -1) if pts.size else np.zeros((0, 3), np.float32)


def _axis_lists(pts, a, ks, dims, lower, upper, res, border):
    """-> (idx [n][len(ks)] int64, ok [n][len(ks)] bool) along axis a; pts float32 [n][>= 3], all finite"""
    inv = 1.0 / res
    coord = pts[:, a].astype(np.float64)[:, None] + ks.astype(np.float64)[None, :] * res  # the product is rounded, then the sum
    q = (coord - lower[a]) * inv
    if border == CLAMP:  # min(max(int(q), 0), size - 1): int() truncates
        return np.clip(np.trunc(q), 0, dims[a] - 1).astype(np.int64), np.ones(q.shape, bool)
    ok = (coord >= lower[a]) & (coord < upper[a])
    idx = np.where(ok, np.trunc(np.where(ok, q, 0.0)), 0).astype(np.int64)
    ok &= idx < dims[a]  # the reference writes out of bounds here; the contract drops
    return idx, ok


def restate(points, margin, border, dims=DIMS, res=RES, lower=LOWER, upper=UPPER, base=None):
    """-> (map uint8 [X][Y][Z], stats int64 [4]: points, skipped as non-finite, dropped triples, occupied).  base: ADD onto it"""
    pts = _rows(points)[:, :3]
    grid = np.zeros(dims, np.uint8) if base is None else np.array(base, np.uint8)
    fin = np.isfinite(pts).all(axis=1)
    p = pts[fin]
    s, sz = steps(margin, res)
    kxy, kz = np.arange(-s, s + 1), np.arange(-sz, sz + 1)
    ix, okx = _axis_lists(p, 0, kxy, dims, lower, upper, res, border)
    iy, oky = _axis_lists(p, 1, kxy, dims, lower, upper, res, border)
    iz, okz = _axis_lists(p, 2, kz, dims, lower, upper, res, border)
    dropped = 0
    for n in range(0, len(p), 4096):  # chunks bound the size of the product
        sl = slice(n, n + 4096)
        ok = okx[sl, :, None, None] & oky[sl, None, :, None] & okz[sl, None, None, :]
        shape = ok.shape
        bx, by, bz = (np.broadcast_to(i, shape) for i in (ix[sl, :, None, None], iy[sl, None, :, None], iz[sl, None, None, :]))
        grid[bx[ok], by[ok], bz[ok]] = 1
        dropped += int((~ok).sum())
    return grid, np.array([len(pts), int((~fin).sum()), dropped, int((grid == 1).sum())], np.int64)


def triple_loop(points, margin, border, dims=DIMS, res=RES, lower=LOWER, upper=UPPER):
    """The reference's loop nest (TRP:539-568), one voxel at a time; Python floats are C doubles"""
    grid = np.zeros(dims, np.uint8)
    inv = 1.0 / res
    s, sz = steps(margin, res)
    skipped = dropped = 0
    for row in _rows(points):
        pt = [float(row[0]), float(row[1]), float(row[2])]
        if not all(math.isfinite(v) for v in pt):
            skipped += 1
            continue
        for x in range(-s, s + 1):
            for y in range(-s, s + 1):
                for z in range(-sz, sz + 1):
                    inf = [pt[0] + x * res, pt[1] + y * res, pt[2] + z * res]
                    if border == CLAMP:
                        idx = [min(max(int((inf[a] - lower[a]) * inv), 0), dims[a] - 1) for a in range(3)]  # Python's int() takes any finite double
                    else:
                        if any(inf[a] < lower[a] or inf[a] >= upper[a] for a in range(3)):
                            dropped += 1
                            continue
                        idx = [int((inf[a] - lower[a]) * inv) for a in range(3)]
                        if any(idx[a] >= dims[a] for a in range(3)):
                            dropped += 1
                            continue
                    grid[idx[0], idx[1], idx[2]] = 1
    return grid, np.array([len(points), skipped, dropped, int(grid.sum())], np.int64)


def dilate_base_voxel(points, margin, dims=DIMS, res=RES, lower=LOWER):
    """What the reference does NOT compute: the point's own voxel (clamped), dilated by the box of steps, clamped"""
    grid = np.zeros(dims, np.uint8)
    s, sz = steps(margin, res)
    pts = np.asarray(points, np.float32)[:, :3]
    base = np.clip(np.trunc((pts.astype(np.float64) - lower) * (1.0 / res)), 0, np.array(dims) - 1).astype(np.int64)
    for b in base:
        lo = np.maximum(b - (s, s, sz), 0)
        hi = np.minimum(b + (s, s, sz), np.array(dims) - 1)
        grid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = 1
    return grid


HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "map_cloud_math.h"
namespace mc = direct::mapcloud;
// in: int32 X, Y, Z, stride, border, reps, pad, pad; int64 n; float64 lower[3], upper[3], resolution, margin; float32 xyz[n][stride];
//     uint8 base[G] (the map to add onto)
// out: int64 stats[4]; float64 ms (best of reps); uint8 map[G]
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[8];
  long long n;
  double d[8];
  if (!f || fread(h, 4, 8, f) != 8 || fread(&n, 8, 1, f) != 1 || fread(d, 8, 8, f) != 8) return 1;
  const int X = h[0], Y = h[1], Z = h[2], stride = h[3], border = h[4], reps = h[5];
  const size_t G = (size_t)X * Y * Z;
  std::vector<float> xyz((size_t)n * stride);
  std::vector<uint8_t> base(G), map(G);
  if (fread(xyz.data(), 4, xyz.size(), f) != xyz.size() || fread(base.data(), 1, G, f) != G) return 1;
  fclose(f);
  const double *lower = d, *upper = d + 3, res = d[6], margin = d[7], inv = 1.0 / res;
  const int size[3] = {X, Y, Z};
  int s, sz;
  mc::inf_steps(margin, res, &s, &sz);
  long long stats[4] = {n, 0, 0, 0};
  double best = 1e300;
  for (int rep = 0; rep < reps; rep++) {
    map = base;
    stats[1] = stats[2] = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (long long p = 0; p < n; p++) {
      const float* pt = &xyz[(size_t)p * stride];
      if (!mc::is_finite3(pt[0], pt[1], pt[2])) { stats[1]++; continue; }
      for (int x = -s; x <= s; x++)
        for (int y = -s; y <= s; y++)
          for (int z = -sz; z <= sz; z++) {
            const int k[3] = {x, y, z};
            int idx[3];
            bool keep = true;
            for (int a = 0; a < 3; a++) {
              idx[a] = mc::axis_index(border, mc::shifted(pt[a], k[a], res), lower[a], upper[a], inv, size[a]);
              keep = keep && idx[a] >= 0;
            }
            if (!keep) { stats[2]++; continue; }
            map[((size_t)idx[0] * Y + idx[1]) * Z + idx[2]] = 1;
          }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms < best) best = ms;
  }
  for (size_t i = 0; i < G; i++) stats[3] += map[i] == 1;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 1;
  fwrite(stats, 8, 4, o);
  fwrite(&best, 8, 1, o);
  fwrite(map.data(), 1, G, o);
  fclose(o);
  return 0;
}
'''


def build(workdir):
    return str(workdir), compile_program(workdir, "map_cloud_harness", HARNESS)


def run(harness, points, margin, border, dims=DIMS, res=RES, lower=LOWER, upper=UPPER, base=None, reps=1):
    """-> (map, stats, ms) of the header program; points float32 [n][3 or 4]"""
    d, exe = harness
    pts = np.ascontiguousarray(_rows(points))
    G = int(np.prod(dims))
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        np.array(list(dims) + [pts.shape[1], border, reps, 0, 0], np.int32).tofile(f)
        np.array([len(pts)], np.int64).tofile(f)
        np.array(list(lower) + list(upper) + [res, margin], np.float64).tofile(f)
        pts.tofile(f)
        (np.zeros(G, np.uint8) if base is None else np.ascontiguousarray(base, np.uint8)).tofile(f)
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        stats = np.fromfile(f, np.int64, 4)
        ms = float(np.fromfile(f, np.float64, 1)[0])
        grid = np.fromfile(f, np.uint8, G).reshape(dims)
        assert f.read() == b""
    os.remove(fout)
    return grid, stats, ms


# ---- the inputs the CPU and the GPU tests share --------------------------------------------------------------------------

def cloud_random(n=2000, dims=DIMS, res=RES, lower=LOWER, seed=1):
    """(a) random float32 points over the map and half a metre around it"""
    rng = np.random.default_rng(seed)
    size = np.array(dims) * res
    return (lower - 0.5 + rng.random((n, 3)) * (size + 1.0)).astype(np.float32)


def cloud_faces(dims=DIMS, res=RES, lower=LOWER):
    """(b) 24 isolated points whose float32 coordinates sit on voxel faces (lower + i * res, rounded to float32), far enough
    apart that their boxes do not touch at any of MARGINS.  Most such faces behave like interior points; y face 18 (float32(0.0)
    against the double -2.7 + 18 * 0.15 and the rounded steps around it) and x face 5 are among those that do not."""
    pts = [[lower[0] + i * res, lower[1] + j * res, lower[2] + k * res] for i in (5, 14, 23, 32) for j in (6, 18, 29) for k in (3, 8)]
    return np.array(pts, np.float64).astype(np.float32)


def cloud_borders(dims=DIMS, res=RES, lower=LOWER, upper=UPPER):
    """(c) for every face of the map: points at several depths within the widest margin inside it, on it, and beyond it -
    among them the gap between the last voxel's far side and the upper corner, and the map's corners"""
    size = np.array(dims) * res
    mid = lower + 0.5 * size + np.array([0.02, 0.03, 0.01])
    pts = []
    for a in range(3):
        for face, sign in ((lower[a], 1.0), (lower[a] + size[a], -1.0), (upper[a], -1.0)):
            for depth in (0.45, 0.31, 0.2, 0.1, 0.04, 0.0, -0.01, -0.04, -0.1, -0.2, -0.31, -0.5, -1.0):
                p = mid.copy()
                p[a] = face + sign * depth
                pts.append(p)
    for cx in (lower[0] + 0.05, lower[0] + size[0] - 0.05, lower[0] - 0.2, lower[0] + size[0] + 0.2):
        for cy in (lower[1] + 0.05, lower[1] + size[1] + 0.1):
            for cz in (lower[2] - 0.05, lower[2] + size[2] - 0.01, lower[2] + size[2] + 0.02):
                pts.append([cx, cy, cz])
    # lone points beyond a face by more than the widest margin, away from all the others: only "clamp" marks anything for them
    pts.append([lower[0] - 1.0, lower[1] + 0.25 * size[1], lower[2] + 0.6 * size[2]])
    pts.append([lower[0] + 0.25 * size[0], upper[1] + 1.0, lower[2] + 0.3 * size[2]])
    pts.append([lower[0] + 0.75 * size[0], lower[1] + 0.75 * size[1], upper[2] + 1.0])
    return np.array(pts, np.float64).astype(np.float32)


def cloud_nonfinite(dims=DIMS, res=RES, lower=LOWER):
    """(d) finite points with NaN and +/-inf rows between them, and one coordinate of 1e30 (finite: it is not skipped)"""
    p = cloud_random(40, dims, res, lower, seed=2)
    p[3, 0] = np.nan
    p[7, 1] = np.inf
    p[8, 2] = -np.inf
    p[12] = [np.nan, np.inf, -np.inf]
    p[20, 2] = np.nan
    p[25, 0] = 1e30
    p[26, 1] = -1e30
    return p


def clouds():
    return dict(random=cloud_random(), faces=cloud_faces(), borders=cloud_borders(), nonfinite=cloud_nonfinite())


def with_stride4(points, fill=7.5):
    """the same points as a pcl::PointXYZ buffer lies in memory: a fourth float that must not be read"""
    p = np.full((len(points), 4), fill, np.float32)
    p[:, :3] = points
    p[::3, 3] = np.nan
    return p
