"""TEST INFRASTRUCTURE of tests/test_evidence_restatement.py, tests/test_gpu_evidence.py and tools/evidence_bench.py: what one
direct_cluster_map_integrate_scan_evidence call (include/direct_cluster.h, "occupancy evidence per voxel") must leave, twice over.
  restate      written from the definition's TEXT and not from direct_amd/csrc/map_evidence_math.h: the touch grid by
               map_scan_harness.walk per point (all passes, then all hits), the fold in NumPy in int32, map_scan_harness.dilate, and
               the twelve stats.
  build / run  a g++ -O2 -ffp-contract=off program with its own main around map_scan_math.h and map_evidence_math.h that emulates
               the three kernels as lane loops on one thread - the fold in groups of 16 voxels with the tail, storing a group only
               where it changed, on buffers of exactly G bytes; it also times itself, for the bench tool.
               build(..., sanitize=True) is the same program under -fsanitize=address,undefined, run stand-alone.
  refusal      the message me::refusal gives a parameter set (the function the library calls), through the same program.
There is no reference counterpart."""
import math
import os
import subprocess

import numpy as np

from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh
from tests.cpp_program import compile_program

DIMS, RES, LOWER, UPPER, ORIGIN, RANGES = sh.DIMS, sh.RES, sh.LOWER, sh.UPPER, sh.ORIGIN, sh.RANGES
STATS = sh.STATS + ("touched_hit", "touched_pass", "positive", "negative")
DEFAULTS = dict(hit=17, miss=8, ev_min=-40, ev_max=70, occ=1)    # the Python binding's: OctoMap's numbers in units of 0.05
SMALL = dict(hit=2, miss=1, ev_min=-3, ev_max=5, occ=3)
LAST_WINS = dict(hit=1, miss=1, ev_min=0, ev_max=1, occ=1)       # the plain scan as a special case
MODES = {"reset": 0, "continue": 1, "adopt": 2}


def touch_grid(points, origin, max_range, dims=DIMS, res=RES, lower=LOWER, upper=UPPER):
    """-> (touch uint8: 0, 1 passed, 2 hit; skipped, truncated, outside).  Step 2 after step 1."""
    pts = mh._rows(points)[:, :3]
    touch = np.zeros(dims, np.uint8)
    skipped = truncated = outside = 0
    inv = 1.0 / float(res)
    hits = []
    for p in pts:
        kind, passed, _ = sh.walk(p, origin, max_range, dims, res, lower, upper)
        skipped += kind == sh.SKIPPED
        truncated += kind == sh.TRUNCATED
        for v in passed:
            touch[v] = 1
        if kind == sh.HIT:
            j = tuple(int(math.floor((float(p[a]) - float(lower[a])) * inv)) for a in range(3))
            if all(0 <= j[a] < dims[a] for a in range(3)):
                hits.append(j)
            else:
                outside += 1
    for j in hits:
        touch[j] = 2
    return touch, skipped, truncated, outside


def fold(ev, touch, par):
    """Step 3 on whole grids, in int32"""
    e = np.asarray(ev).astype(np.int32)
    up = np.minimum(e + par["hit"], par["ev_max"])
    down = np.maximum(e - par["miss"], par["ev_min"])
    return np.where(touch == 2, up, np.where(touch == 1, down, e))


def restate(points, origin, max_range, par=DEFAULTS, inflate=(0, 0, 0), mode="continue", ev=None, before=None, known=None, track=False,
            dims=DIMS, res=RES, lower=LOWER, upper=UPPER, touched=None):
    """One evidence scan.  ev: the evidence grid the handle holds (None: none); before: the map it holds (None: none, all 0);
    known: its known grid (None: none); touched: touch_grid's result for these points, where a test shares it between cases.
    -> dict(ev int8, raw, map, known (None when untracked), stats int64 [12], touch)"""
    pts = mh._rows(points)[:, :3]
    old = np.zeros(dims, np.uint8) if before is None else np.asarray(before, np.uint8)
    if mode == "reset":
        e0 = np.zeros(dims, np.int32)
    elif mode == "continue":
        e0 = np.zeros(dims, np.int32) if ev is None else np.asarray(ev).astype(np.int32)
    else:
        assert before is not None
        e0 = np.where(old == 1, par["ev_max"], 0).astype(np.int32)
    touch, skipped, truncated, outside = touched if touched is not None else touch_grid(pts, origin, max_range, dims, res, lower, upper)
    e = fold(e0, touch, par)
    assert e.min() >= -127 and e.max() <= 127
    raw = (e >= par["occ"]).astype(np.uint8)
    new = sh.dilate(raw, inflate)
    kn = None
    if track:
        kn = np.zeros(dims, np.uint8) if known is None or mode == "reset" else (np.asarray(known) != 0).astype(np.uint8)
        kn = kn | (touch != 0).astype(np.uint8)
    stats = [len(pts), skipped, truncated, outside, int(raw.sum()), int(new.sum()), int(((old != new) & (new == 1)).sum()),
             int(((old != new) & (new == 0)).sum()), int((touch == 2).sum()), int((touch == 1).sum()), int((e > 0).sum()), int((e < 0).sum())]
    return dict(ev=e.astype(np.int8), raw=raw, map=new, known=kn, stats=np.array(stats, np.int64), touch=touch)


HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "map_scan_math.h"
#include "map_evidence_math.h"
namespace mc = direct::mapcloud;
namespace ms = direct::mapscan;
namespace me = direct::mapevid;
// --refusal hit miss ev_min ev_max occ r0 r1 r2: prints me::refusal's message, or "ok"
// in: int32 X, Y, Z, stride, inflate[3], mode, track, lanes, hit, miss, ev_min, ev_max, occ, reps; int64 n;
//     float64 lower[3], upper[3], resolution, max_range, origin[3]; float32 xyz[n][stride]; int8 ev[G]; uint8 raw[G] (the scan grid
//     the handle holds), before[G] (its map), known[G]
// out: int64 stats[12]; float64 ms (best of reps); int8 ev[G]; uint8 raw[G], map[G], known[G].  Exit status 3: the origin lies
// outside the map
int main(int argc, char** argv) {
  if (argc == 10 && !strcmp(argv[1], "--refusal")) {
    me::Params P = {atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
    const int32_t r[3] = {atoi(argv[7]), atoi(argv[8]), atoi(argv[9])};
    const char* why = me::refusal(P, r);
    printf("%s\n", why ? why : "ok");
    return 0;
  }
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[16];
  long long n;
  double d[11];
  if (!f || fread(h, 4, 16, f) != 16 || fread(&n, 8, 1, f) != 1 || fread(d, 8, 11, f) != 11) return 1;
  const int stride = h[3], mode = h[7], track = h[8], lanes = h[9], reps = h[15];
  const int size[3] = {h[0], h[1], h[2]}, inflate[3] = {h[4], h[5], h[6]};
  const me::Params P = {h[10], h[11], h[12], h[13], h[14]};
  const size_t G = (size_t)size[0] * size[1] * size[2];
  std::vector<float> xyz((size_t)n * stride);
  std::vector<int8_t> ev0(G), ev(G);
  std::vector<uint8_t> raw0(G), before(G), known0(G), raw(G), known(G), touch(G), tmp[2], map(G);
  if (fread(xyz.data(), 4, xyz.size(), f) != xyz.size() || fread(ev0.data(), 1, G, f) != G || fread(raw0.data(), 1, G, f) != G ||
      fread(before.data(), 1, G, f) != G || fread(known0.data(), 1, G, f) != G)
    return 1;
  fclose(f);
  ms::Grid Gd;
  Gd.resolution = d[6]; Gd.inv = 1.0 / d[6]; Gd.R2 = d[7] * d[7];
  for (int a = 0; a < 3; a++) {
    Gd.lower[a] = d[a]; Gd.origin[a] = d[8 + a]; Gd.size[a] = size[a];
    Gd.start[a] = mc::axis_index_drop(d[8 + a], d[a], d[3 + a], Gd.inv, size[a]);
    if (Gd.start[a] < 0) return 3;
  }
  tmp[0].resize(G); tmp[1].resize(G);
  long long stats[12] = {n};
  double best = 1e300;
  for (int rep = 0; rep < reps; rep++) {
    ev = ev0; raw = raw0; known = known0;
    if (mode == 0) std::fill(ev.begin(), ev.end(), (int8_t)0);          // RESET; ADOPT is served by the fold
    if (mode == 0 && track) std::fill(known.begin(), known.end(), (uint8_t)0);
    std::fill(touch.begin(), touch.end(), (uint8_t)0);
    for (int k = 1; k < 12; k++) stats[k] = 0;
    const auto t0 = std::chrono::steady_clock::now();
    uint8_t* t = touch.data();
    for (int lane = 0; lane < lanes; lane++)          // k_evid_touch: a lane owns the rays lane, lane + lanes, ...
      for (long long p = lane; p < n; p += lanes) {
        const float* q = &xyz[(size_t)p * stride];
        const int kind = ms::carve_ray(Gd, q[0], q[1], q[2], [t](size_t at) { if (t[at] != me::kPass) t[at] = me::kPass; });
        stats[1] += kind == ms::kSkipped;
        stats[2] += kind == ms::kTruncated;
      }
    for (int lane = 0; lane < lanes; lane++)          // k_evid_hit
      for (long long p = lane; p < n; p += lanes) {
        const float* q = &xyz[(size_t)p * stride];
        size_t at = 0;
        const int m = ms::mark_voxel(Gd, q[0], q[1], q[2], &at);
        if (m > 0) t[at] = me::kHit;
        stats[3] += m < 0;
      }
    const long long groups = ((long long)G + 15) / 16;
    for (int lane = 0; lane < lanes; lane++)          // k_evid_fold: a lane owns groups of 16 voxels; the last group may be short
      for (long long g = lane; g < groups; g += lanes) {
        const size_t at = (size_t)g * 16;
        const int cnt = G - at < 16 ? (int)(G - at) : 16;
        uint8_t tk[16], e0[16], r0[16], k0[16] = {0}, e1[16], r1[16], k1[16];
        memcpy(tk, &touch[at], cnt);
        memcpy(e0, mode == 2 ? (const void*)&before[at] : (const void*)&ev[at], cnt);
        memcpy(r0, &raw[at], cnt);
        if (track) memcpy(k0, &known[at], cnt);
        for (int k = 0; k < cnt; k++) {
          const int was = mode == 2 ? me::adopt(e0[k], P) : (int)(int8_t)e0[k];
          const int e = me::fold(was, tk[k], P);
          e1[k] = (uint8_t)(int8_t)e;
          r1[k] = me::occupied(e, P);
          k1[k] = k0[k] | (tk[k] != me::kNone);
          stats[8] += tk[k] == me::kHit;
          stats[9] += tk[k] == me::kPass;
          stats[10] += e > 0;
          stats[11] += e < 0;
        }
        if (mode == 2 || memcmp(e0, e1, cnt)) memcpy(&ev[at], e1, cnt);
        if (memcmp(r0, r1, cnt)) memcpy(&raw[at], r1, cnt);
        if (track && memcmp(k0, k1, cnt)) memcpy(&known[at], k1, cnt);
      }
    const uint8_t* src = raw.data();  // k_scan_dilate: z, y where they inflate, x last
    for (int axis = 2; axis >= 0; axis--) {
      if (axis > 0 && inflate[axis] == 0) continue;
      uint8_t* dst = axis == 0 ? map.data() : tmp[axis - 1].data();
      size_t u = 0;
      for (int x = 0; x < size[0]; x++)
        for (int y = 0; y < size[1]; y++)
          for (int z = 0; z < size[2]; z++, u++) {
            const int v[3] = {x, y, z};
            dst[u] = ms::dilate_at(src, size, axis, inflate[axis], v);
          }
      src = dst;
    }
    for (size_t u = 0; u < G; u++) {
      stats[4] += raw[u] == 1;
      stats[5] += map[u] == 1;
      stats[6] += before[u] != map[u] && map[u] == 1;
      stats[7] += before[u] != map[u] && map[u] == 0;
    }
    const double ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms_ < best) best = ms_;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 1;
  fwrite(stats, 8, 12, o);
  fwrite(&best, 8, 1, o);
  fwrite(ev.data(), 1, G, o);
  fwrite(raw.data(), 1, G, o);
  fwrite(map.data(), 1, G, o);
  fwrite(known.data(), 1, G, o);
  fclose(o);
  return 0;
}
'''


def build(workdir, sanitize=False):
    name = "evidence_harness_san" if sanitize else "evidence_harness"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    return str(workdir), compile_program(workdir, name, HARNESS, extra)


def refusal(harness, hit, miss, ev_min, ev_max, occ, reserved=(0, 0, 0)):
    """-> the message a parameter set is refused with, or 'ok'"""
    args = [str(int(v)) for v in (hit, miss, ev_min, ev_max, occ) + tuple(reserved)]
    return subprocess.check_output([harness[1], "--refusal"] + args, text=True).strip()


def run(harness, points, origin, max_range, par=DEFAULTS, inflate=(0, 0, 0), mode="continue", ev=None, raw=None, before=None, known=None,
        track=False, lanes=64, dims=DIMS, res=RES, lower=LOWER, upper=UPPER, reps=1):
    """-> dict(ev, raw, map, known (None when untracked), stats, ms) of the header program; points float32 [n][3 or 4]"""
    d, exe = harness
    pts = np.ascontiguousarray(mh._rows(points))
    G = int(np.prod(dims))
    tag = os.path.basename(exe)
    fin, fout = os.path.join(d, tag + "_in.bin"), os.path.join(d, tag + "_out.bin")
    with open(fin, "wb") as f:
        np.array(list(dims) + [pts.shape[1]] + [int(v) for v in inflate] + [MODES[mode], int(track), int(lanes)] +
                 [par[k] for k in ("hit", "miss", "ev_min", "ev_max", "occ")] + [reps], np.int32).tofile(f)
        np.array([len(pts)], np.int64).tofile(f)
        np.array(list(lower) + list(upper) + [res, max_range] + list(origin), np.float64).tofile(f)
        pts.tofile(f)
        (np.zeros(G, np.int8) if ev is None else np.ascontiguousarray(ev, np.int8)).tofile(f)
        for g in (raw, before, known):
            (np.zeros(G, np.uint8) if g is None else np.ascontiguousarray(g, np.uint8)).tofile(f)
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        stats = np.fromfile(f, np.int64, 12)
        ms = float(np.fromfile(f, np.float64, 1)[0])
        e = np.fromfile(f, np.int8, G).reshape(dims)
        grid = np.fromfile(f, np.uint8, G).reshape(dims)
        new = np.fromfile(f, np.uint8, G).reshape(dims)
        kn = np.fromfile(f, np.uint8, G).reshape(dims)
        assert f.read() == b""
    os.remove(fout)
    return dict(ev=e, raw=grid, map=new, known=kn if track else None, stats=stats, ms=ms)


def same(a, b, what=("ev", "raw", "map", "known", "stats")):
    """every grid and every stat of two results, for equality"""
    for k in what:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (k, a["stats"], b["stats"])
