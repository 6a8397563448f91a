"""TEST INFRASTRUCTURE of tests/test_map_scan_restatement.py, tests/test_gpu_map_scan.py and tools/map_scan_bench.py: what one
direct_cluster_map_integrate_scan call (include/direct_cluster.h, "one sensor scan folded into the map") must leave, twice over.
  restate      pure Python floats (which are C doubles, with no fused multiply-add), written from the definition's TEXT and not
               from direct_amd/csrc/map_scan_math.h: the walk of every ray, the carve phase, then the mark phase, then the
               inflation by shifted ORs in NumPy, and the eight stats.  walk() alone gives one ray's voxels for the geometric check.
  build / run  a g++ -O2 -ffp-contract=off program with its own main around map_scan_math.h that emulates the three kernels as
               lane loops on one thread (the pattern of tests/map_cloud_harness.py); it also times itself, for the bench tool.
               build(..., sanitize=True) is the same program under -fsanitize=address,undefined, run stand-alone.
There is no reference counterpart: the reference builds its map once and never takes a voxel out again."""
import math
import os
import subprocess

import numpy as np

from tests import map_cloud_harness as mh
from tests.cpp_program import compile_program

ROOT = mh.ROOT
DIMS, RES, LOWER, UPPER = mh.DIMS, mh.RES, mh.LOWER, mh.UPPER   # 40 x 36 x 12 voxels of 0.15 m
ORIGIN = np.array([0.3125, -0.21875, 0.90625])   # float32 numbers in the open interior of voxel (22, 16, 6)
RANGES = (0.6, 1.5, 10.0)
SKIPPED, HIT, TRUNCATED = 0, 1, 2
STATS = ("points", "skipped_nonfinite", "truncated", "outside", "raw_occupied", "occupied", "set", "cleared")


def origin_voxel(origin, dims, res, lower, upper):
    """axis_index_drop per axis: None when the origin is outside [lower, upper) or beyond the last voxel"""
    inv = 1.0 / res
    v = []
    for a in range(3):
        c = float(origin[a])
        if not (c >= lower[a]) or not (c < upper[a]):
            return None
        q = (c - float(lower[a])) * inv
        if not (q < dims[a]):
            return None
        v.append(int(q))
    return v


def walk(p, origin, max_range, dims=DIMS, res=RES, lower=LOWER, upper=UPPER):
    """One ray.  -> (kind, cleared: the voxels the carve writes, in order; end: where a hit's walk stands when it stops)"""
    e = [float(p[0]), float(p[1]), float(p[2])]
    if not all(math.isfinite(v) for v in e):
        return SKIPPED, [], None
    res, inv, R2 = float(res), 1.0 / float(res), float(max_range) * float(max_range)
    o = [float(v) for v in origin]
    lo = [float(v) for v in lower]
    d = [e[a] - o[a] for a in range(3)]
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    hit = dd <= R2
    i = origin_voxel(origin, dims, res, lower, upper)
    step = [(v > 0.0) - (v < 0.0) for v in d]
    n, tmax, tdel = [0, 0, 0], [None] * 3, [None] * 3
    for a in range(3):
        if hit:
            n[a] = abs(int(math.floor((e[a] - lo[a]) * inv)) - i[a])
        if step[a] != 0:
            b = lo[a] + float(i[a] + (1 if step[a] > 0 else 0)) * res
            tmax[a] = (b - o[a]) / d[a]
            tdel[a] = res / abs(d[a])
    cleared = []
    left = sum(n) if hit else sum(dims)
    while all(0 <= i[a] < dims[a] for a in range(3)):
        if left == 0:
            break
        c = None
        for a in range(3):
            if step[a] != 0 and (not hit or n[a] > 0) and (c is None or tmax[a] < tmax[c]):
                c = a
        assert c is not None
        cleared.append(tuple(i))
        t = tmax[c]
        if not hit and not ((t * t) * dd <= R2):
            break
        i[c] += step[c]
        tmax[c] += tdel[c]
        n[c] -= 1
        left -= 1
    return (HIT if hit else TRUNCATED), cleared, (tuple(i) if hit else None)


def dilate(raw, inflate):
    """The voxel box without wrap, by shifted ORs along each axis in turn"""
    out = (np.asarray(raw) == 1)
    for a in range(3):
        src, acc = out, out.copy()
        for k in range(1, min(int(inflate[a]), src.shape[a] - 1) + 1):
            fwd = [slice(None)] * 3
            back = [slice(None)] * 3
            fwd[a], back[a] = slice(k, None), slice(None, -k)
            acc[tuple(fwd)] |= src[tuple(back)]
            acc[tuple(back)] |= src[tuple(fwd)]
        out = acc
    return out.astype(np.uint8)


def restate(points, origin, max_range, inflate=(0, 0, 0), raw=None, before=None, dims=DIMS, res=RES, lower=LOWER, upper=UPPER):
    """One scan call.  raw: the scan grid the call starts from (None: empty); before: the map the handle held (None: none, all 0).
    -> (raw, map, stats int64 [8])"""
    pts = mh._rows(points)[:, :3]
    grid = np.zeros(dims, np.uint8) if raw is None else np.array(raw, np.uint8)
    old = np.zeros(dims, np.uint8) if before is None else np.asarray(before, np.uint8)
    skipped = truncated = outside = 0
    inv = 1.0 / float(res)
    marks = []
    for p in pts:
        kind, cleared, _ = walk(p, origin, max_range, dims, res, lower, upper)
        skipped += kind == SKIPPED
        truncated += kind == TRUNCATED
        for v in cleared:
            grid[v] = 0
        if kind == HIT:
            j = tuple(int(math.floor((float(p[a]) - float(lower[a])) * inv)) for a in range(3))
            if all(0 <= j[a] < dims[a] for a in range(3)):
                marks.append(j)
            else:
                outside += 1
    for j in marks:  # all carving precedes all marking
        grid[j] = 1
    new = dilate(grid, inflate)
    stats = [len(pts), skipped, truncated, outside, int((grid == 1).sum()), int((new == 1).sum()),
             int(((old != new) & (new == 1)).sum()), int(((old != new) & (new == 0)).sum())]
    return grid, new, np.array(stats, np.int64)


HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "map_scan_math.h"
namespace mc = direct::mapcloud;
namespace ms = direct::mapscan;
// in: int32 X, Y, Z, stride, inflate[3], reps; int64 n; float64 lower[3], upper[3], resolution, max_range, origin[3];
//     float32 xyz[n][stride]; uint8 raw[G] (the scan grid to start from), before[G] (the map the handle held)
// out: int64 stats[8]; float64 ms (best of reps); uint8 raw[G], map[G].  Exit status 3: the origin lies outside the map
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[8];
  long long n;
  double d[11];
  if (!f || fread(h, 4, 8, f) != 8 || fread(&n, 8, 1, f) != 1 || fread(d, 8, 11, f) != 11) return 1;
  const int stride = h[3], reps = h[7];
  const int size[3] = {h[0], h[1], h[2]}, inflate[3] = {h[4], h[5], h[6]};
  const size_t G = (size_t)size[0] * size[1] * size[2];
  std::vector<float> xyz((size_t)n * stride);
  std::vector<uint8_t> raw0(G), before(G), raw(G), tmp[2], map(G);
  if (fread(xyz.data(), 4, xyz.size(), f) != xyz.size() || fread(raw0.data(), 1, G, f) != G || fread(before.data(), 1, G, f) != G) return 1;
  fclose(f);
  ms::Grid Gd;
  Gd.resolution = d[6]; Gd.inv = 1.0 / d[6]; Gd.R2 = d[7] * d[7];
  for (int a = 0; a < 3; a++) {
    Gd.lower[a] = d[a]; Gd.origin[a] = d[8 + a]; Gd.size[a] = size[a];
    Gd.start[a] = mc::axis_index_drop(d[8 + a], d[a], d[3 + a], Gd.inv, size[a]);
    if (Gd.start[a] < 0) return 3;
  }
  tmp[0].resize(G); tmp[1].resize(G);
  long long stats[8] = {n, 0, 0, 0, 0, 0, 0, 0};
  double best = 1e300;
  for (int rep = 0; rep < reps; rep++) {
    raw = raw0;
    for (int k = 1; k < 8; k++) stats[k] = 0;
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t* g = raw.data();
    for (long long p = 0; p < n; p++) {  // k_scan_carve, one lane after the other
      const float* q = &xyz[(size_t)p * stride];
      const int kind = ms::carve_ray(Gd, q[0], q[1], q[2], [g](size_t at) { g[at] = 0; });
      stats[1] += kind == ms::kSkipped;
      stats[2] += kind == ms::kTruncated;
    }
    for (long long p = 0; p < n; p++) {  // k_scan_mark
      const float* q = &xyz[(size_t)p * stride];
      size_t at = 0;
      const int m = ms::mark_voxel(Gd, q[0], q[1], q[2], &at);
      if (m > 0) g[at] = 1;
      stats[3] += m < 0;
    }
    const uint8_t* src = g;  // k_scan_dilate: z, y where they inflate, x last
    for (int axis = 2; axis >= 0; axis--) {
      if (axis > 0 && inflate[axis] == 0) continue;
      uint8_t* dst = axis == 0 ? map.data() : tmp[axis - 1].data();
      size_t t = 0;
      for (int x = 0; x < size[0]; x++)
        for (int y = 0; y < size[1]; y++)
          for (int z = 0; z < size[2]; z++, t++) {
            const int v[3] = {x, y, z};
            dst[t] = ms::dilate_at(src, size, axis, inflate[axis], v);
          }
      src = dst;
    }
    for (size_t t = 0; t < G; t++) {
      stats[4] += g[t] == 1;
      stats[5] += map[t] == 1;
      stats[6] += before[t] != map[t] && map[t] == 1;
      stats[7] += before[t] != map[t] && map[t] == 0;
    }
    const double ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms_ < best) best = ms_;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 1;
  fwrite(stats, 8, 8, o);
  fwrite(&best, 8, 1, o);
  fwrite(raw.data(), 1, G, o);
  fwrite(map.data(), 1, G, o);
  fclose(o);
  return 0;
}
'''


def build(workdir, sanitize=False):
    name = "map_scan_harness_san" if sanitize else "map_scan_harness"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    return str(workdir), compile_program(workdir, name, HARNESS, extra)


def run(harness, points, origin, max_range, inflate=(0, 0, 0), raw=None, before=None, dims=DIMS, res=RES, lower=LOWER, upper=UPPER,
        reps=1):
    """-> (raw, map, stats, ms) of the header program; points float32 [n][3 or 4]"""
    d, exe = harness
    pts = np.ascontiguousarray(mh._rows(points))
    G = int(np.prod(dims))
    tag = os.path.basename(exe)
    fin, fout = os.path.join(d, tag + "_in.bin"), os.path.join(d, tag + "_out.bin")
    with open(fin, "wb") as f:
        np.array(list(dims) + [pts.shape[1]] + [int(v) for v in inflate] + [reps], np.int32).tofile(f)
        np.array([len(pts)], np.int64).tofile(f)
        np.array(list(lower) + list(upper) + [res, max_range] + list(origin), np.float64).tofile(f)
        pts.tofile(f)
        for g in (raw, before):
            (np.zeros(G, np.uint8) if g is None else np.ascontiguousarray(g, np.uint8)).tofile(f)
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        stats = np.fromfile(f, np.int64, 8)
        ms = float(np.fromfile(f, np.float64, 1)[0])
        grid = np.fromfile(f, np.uint8, G).reshape(dims)
        new = np.fromfile(f, np.uint8, G).reshape(dims)
        assert f.read() == b""
    os.remove(fout)
    return grid, new, stats, ms


# ---- the inputs the CPU and the GPU tests share --------------------------------------------------------------------------

def cloud_lattice(dims=DIMS, res=RES, lower=LOWER):
    """every coordinate of every endpoint on a voxel face: lower + i * res, rounded to float32"""
    pts = [[lower[0] + i * res, lower[1] + j * res, lower[2] + k * res]
           for i in range(0, dims[0] + 1, 3) for j in range(0, dims[1] + 1, 3) for k in range(0, dims[2] + 1, 2)]
    return np.array(pts, np.float64).astype(np.float32)


def cloud_axis_parallel(origin=ORIGIN):
    """rays along +/-x, +/-y and +/-z (two coordinates equal the origin's exactly), short, long and beyond the map; then the
    origin itself"""
    pts = []
    for a in range(3):
        for s in (-7.0, -2.0, -0.6, -0.31, -0.15, -0.01, 0.01, 0.15, 0.3, 0.6, 1.1, 2.0, 7.0):
            p = np.array(origin, np.float64)
            p[a] += s
            pts.append(p)
    pts.append(np.array(origin, np.float64))
    return np.array(pts, np.float64).astype(np.float32)


def clouds():
    """random points over the map and half a metre around it; lattice points; axis-parallel rays and the origin itself; points
    inside, on and outside each of the six faces; non-finite rows.  Against RANGES every cloud has hits, truncated rays and (the
    origin is 1 m from the z faces) truncated rays that leave the map before their range ends."""
    return dict(random=mh.cloud_random(1000), lattice=cloud_lattice(), axis=cloud_axis_parallel(), borders=mh.cloud_borders(),
                nonfinite=mh.cloud_nonfinite())


def wall_and_room(origin=ORIGIN, dims=DIMS, res=RES, lower=LOWER):
    """-> (wall points, room points, wall voxels [n][3]): a patch of the plane x = 28 in front of the origin at voxel centres, and
    the plane x = 36 behind it sampled every half voxel over the whole map, whose rays cover the patch"""
    wall = np.array([[28, y, z] for y in range(12, 22) for z in range(5, 8)])
    wpts = (lower + (wall + 0.5) * res).astype(np.float32)
    y, z = np.meshgrid(np.arange(0.25, dims[1], 0.5), np.arange(0.25, dims[2], 0.5), indexing="ij")
    room = np.stack([np.full(y.size, 36.5), y.ravel(), z.ravel()], axis=1)
    return wpts, (lower + room * res).astype(np.float32), wall
