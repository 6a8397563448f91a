"""Known space and frontier goals (include/direct_cluster.h, "known space and frontier goals") - TEST INFRASTRUCTURE of
tests/test_frontier_restatement.py and tests/test_gpu_frontier.py.  Two sides:
  known_restate / components / select   an independent NumPy restatement: the known grid from the cleared lists of
                                        map_scan_harness.walk plus the marks; the frontier predicate by shifted comparisons, labels
                                        and sizes from free_comp_harness.restate's flood fill on the mask, centroid and
                                        representative by the integer formulas in Python ints.
  build / run_scan / run_frontier       map_scan_math.h, free_comp_math.h and frontier_math.h compiled by g++ into ONE stand-alone
                                        program that emulates the tracked carve and mark, the mask, the labelling, the ordered
                                        compaction, the sums and the representative choice as lane loops on one thread.
                                        build(..., sanitize=True) is the same program under -fsanitize=address,undefined.
and the scenes the CPU and GPU tests share.  There is no reference counterpart."""
import math
import os
import subprocess

import numpy as np

from tests import free_comp_harness as fh
from tests import map_scan_harness as sh
from tests.cpp_program import compile_program

ROOT = sh.ROOT
STATS = ("known", "frontier", "components", "kept", "written", "largest")
RESET, CONTINUE, ADOPT = 0, 1, 2


# ---- the NumPy restatement -----------------------------------------------------------------------------------------------
def known_restate(points, origin, max_range, known=None, dims=sh.DIMS, res=sh.RES, lower=sh.LOWER, upper=sh.UPPER):
    """The known grid after one tracked scan that started from `known` (None: empty): every voxel a ray's walk clears and every
    voxel a hit inside the map marks is 1"""
    out = np.zeros(dims, np.uint8) if known is None else np.array(known, np.uint8)
    inv = 1.0 / float(res)
    for p in sh.mh._rows(points)[:, :3]:
        kind, cleared, _ = sh.walk(p, origin, max_range, dims, res, lower, upper)
        for v in cleared:
            out[v] = 1
        if kind == sh.HIT:
            j = tuple(int(math.floor((float(p[a]) - float(lower[a])) * inv)) for a in range(3))
            if all(0 <= j[a] < dims[a] for a in range(3)):
                out[j] = 1
    return out


def frontier_voxels(grid, known, d2=None, min_d2=0):
    """known, enterable, and a face neighbour INSIDE the map that is not known - by shifted comparisons"""
    kn = np.asarray(known) != 0
    unseen = np.zeros(kn.shape, bool)
    for a in range(3):
        fwd, back = [slice(None)] * 3, [slice(None)] * 3
        fwd[a], back[a] = slice(1, None), slice(None, -1)
        unseen[tuple(back)] |= ~kn[tuple(fwd)]   # the neighbour at +1
        unseen[tuple(fwd)] |= ~kn[tuple(back)]   # the neighbour at -1
    return kn & fh.enterable(grid, d2, min_d2) & unseen


def components(grid, known, d2=None, min_d2=0):
    """Everything of a scene that does not depend on min_size and capacity, computed ONCE and shared.
    -> dict(front, label, size, roots: per component in ascending label order (label, size, centroid, rep, tie, centroid_member),
    known: the count)"""
    front = frontier_voxels(grid, known, d2, min_d2)
    label, size, _ = fh.restate((~front).astype(np.uint8))
    X, Y, Z = front.shape
    lab = label.reshape(-1)
    members = {}
    for v in np.flatnonzero(lab >= 0).tolist():
        members.setdefault(int(lab[v]), []).append(v)
    roots = []
    for r in sorted(members):
        vox = [(v // (Y * Z), (v // Z) % Y, v % Z, v) for v in members[r]]
        n = len(vox)
        c = tuple((2 * sum(q[a] for q in vox) + n) // (2 * n) for a in range(3))
        keys = sorted((min(sum((q[a] - c[a]) ** 2 for a in range(3)), 0xffffffff), q[3]) for q in vox)
        best = keys[0][1]
        roots.append(dict(label=r, size=n, centroid=c, rep=(best // (Y * Z), (best // Z) % Y, best % Z),
                          tie=len(keys) > 1 and keys[1][0] == keys[0][0],
                          centroid_member=(c[0] * Y + c[1]) * Z + c[2] in members[r]))
    return dict(front=front, label=label, size=size, roots=roots, known=int((np.asarray(known) != 0).sum()))


def select(comp, min_size=1, capacity=1024):
    """-> dict(label, size, centroid, rep, voxel_label, stats[6]) of one call on a scene's components()"""
    kept = [r for r in comp["roots"] if r["size"] >= min_size]
    w = kept[:capacity]
    sizes = [r["size"] for r in comp["roots"]]
    stats = np.array([comp["known"], int(comp["front"].sum()), len(sizes), len(kept), len(w), max(sizes, default=0)], np.int64)
    return dict(label=np.array([r["label"] for r in w], np.int32), size=np.array([r["size"] for r in w], np.int32),
                centroid=np.array([r["centroid"] for r in w], np.int32).reshape(-1, 3),
                rep=np.array([r["rep"] for r in w], np.int32).reshape(-1, 3), voxel_label=comp["label"], stats=stats)


def assert_same(got, want, what=""):
    for k in ("label", "size", "centroid", "rep"):
        g = np.asarray(got[k].cpu() if hasattr(got[k], "cpu") else got[k])
        assert g.dtype == np.int32 and g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k, g, want[k])
    gs = got["stats"]
    gs = [gs[k] for k in STATS] if isinstance(gs, dict) else list(gs)
    assert gs == want["stats"].tolist(), (what, gs, want["stats"])
    if got.get("voxel_label") is not None:
        g = got["voxel_label"]
        g = np.asarray(g.cpu() if hasattr(g, "cpu") else g)
        assert g.dtype == np.int32 and np.array_equal(g, want["voxel_label"]), (what, "voxel_label")


# ---- scenes: (name, map, known) on fh.DIMS ---------------------------------------------------------------------------------
def scenes(dims=fh.DIMS):
    X, Y, Z = dims
    xs, ys, zs = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    free = np.zeros(dims, np.uint8)
    ball = (((xs - X // 2) ** 2 + (ys - Y // 2) ** 2 + ((zs - Z // 2) * 2) ** 2) <= (Y // 2 - 1) ** 2).astype(np.uint8)
    box = np.zeros(dims, np.uint8)
    box[:X // 2 + 1, :Y // 2 + 1, :Z // 2 + 1] = 1          # touches the faces x = 0, y = 0 and z = 0
    rooms, seen = np.zeros(dims, np.uint8), np.zeros(dims, np.uint8)
    rooms[X // 2 - 1:X // 2 + 2] = 1                        # a wall of three layers: its shell is occupied on both sides
    seen[:X // 2 - 1] = 1                                   # the near room is known, the wall and the far room are not
    seen[:3, :3, :] = 0                                     # ... but for a pocket in the corner
    # a checkerboard of period 2 in every axis: no two known voxels touch, every one is a component of its own; in the upper half
    # three-voxel Vs (4i, 3j), (4i + 1, 3j + 1), (4i + 2, 3j), whose centroid voxel (4i + 1, 3j) is no member and 1 from all three
    checker = ((xs % 2 == 0) & (ys % 2 == 0) & (zs % 2 == 0) & (zs < Z // 2)).astype(np.uint8)
    vee = ((xs % 4 == 0) & (ys % 3 == 0)) | ((xs % 4 == 1) & (ys % 3 == 1)) | ((xs % 4 == 2) & (ys % 3 == 0))
    checker |= (vee & (zs % 2 == 0) & (zs >= Z // 2) & (ys < Y - Y % 3)).astype(np.uint8)
    out = [("ball", free, ball), ("box_on_three_faces", free, box), ("two_rooms", rooms, seen), ("checkerboard", free, checker)]
    for seed, density in ((1, 0.5), (2, 0.15), (3, 0.05)):   # a few large components, many small ones, mostly single voxels
        rng = np.random.default_rng(100 + seed)
        out.append(("random_seed%d" % seed, (rng.random(dims) < 0.2).astype(np.uint8), (rng.random(dims) < density).astype(np.uint8) * 3))
    return out


def door_scene(width=3, dims=fh.DIMS):
    """the door map of the free components with the lower half in y known: the frontier is a plane through the door, which a floor
    takes away from the wall and, once the door is not enterable, cuts in two"""
    grid = fh.door_map(width, dims)
    known = np.zeros(dims, np.uint8)
    known[:, :dims[1] // 2] = 1
    return grid, known


# ---- the headers, compiled by g++ ------------------------------------------------------------------------------------------
HARNESS = r'''
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "map_scan_math.h"
#include "free_comp_math.h"
#include "frontier_math.h"
namespace mc = direct::mapcloud;
namespace ms = direct::mapscan;
namespace fc = direct::freecomp;
namespace fr = direct::frontier;

template <typename T> static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
template <typename T> static void wr(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

// op 0, one scan.  in: int32 X, Y, Z, stride, mode, flags, test_store, had_known; int64 n; float64 lower[3], upper[3], resolution,
//   max_range, origin[3]; float32 xyz[n][stride]; uint8 raw[G], known[G] (what the handle held)
// out: int32 refused (1: unknown flags, 3: the origin lies outside the map); int64 stats[4] (points, skipped, truncated, outside);
//   uint8 raw[G]; int32 has_known; uint8 known[G]
static int scan(FILE* fi, FILE* fo) {
  const std::vector<int32_t> h = rd<int32_t>(fi, 8);
  const long long n = rd<int64_t>(fi, 1)[0];
  const std::vector<double> d = rd<double>(fi, 11);
  const int size[3] = {h[0], h[1], h[2]}, stride = h[3], mode = h[4], flags = h[5], test_store = h[6], had_known = h[7];
  const size_t G = (size_t)size[0] * size[1] * size[2];
  const std::vector<float> xyz = rd<float>(fi, (size_t)n * stride);
  std::vector<uint8_t> raw = rd<uint8_t>(fi, G), known = rd<uint8_t>(fi, G);
  ms::Grid Gd;
  Gd.resolution = d[6]; Gd.inv = 1.0 / d[6]; Gd.R2 = d[7] * d[7];
  int32_t refused = ms::flags_known(flags) ? 0 : 1;
  for (int a = 0; a < 3; a++) {
    Gd.lower[a] = d[a]; Gd.origin[a] = d[8 + a]; Gd.size[a] = size[a];
    Gd.start[a] = mc::axis_index_drop(d[8 + a], d[a], d[3 + a], Gd.inv, size[a]);
    if (Gd.start[a] < 0 && !refused) refused = 3;
  }
  fwrite(&refused, 4, 1, fo);
  if (refused) return 0;
  const bool track = (flags & ms::kTrackKnown) != 0;
  if (track && (mode == 0 || !had_known)) std::fill(known.begin(), known.end(), 0);   // RESET, or a handle without a known grid
  std::vector<int64_t> stats = {n, 0, 0, 0};
  uint8_t *g = raw.data(), *k = known.data();
  for (long long p = 0; p < n; p++) {  // k_scan_carve<kTest, kKnown>, one lane after the other
    const float* q = &xyz[(size_t)p * stride];
    const int kind = ms::carve_ray(Gd, q[0], q[1], q[2], [g, k, test_store, track](size_t at) {
      if (!test_store || g[at] != 0) g[at] = 0;
      if (track && (!test_store || k[at] != 1)) k[at] = 1;
    });
    stats[1] += kind == ms::kSkipped;
    stats[2] += kind == ms::kTruncated;
  }
  for (long long p = 0; p < n; p++) {  // k_scan_mark<kKnown>
    const float* q = &xyz[(size_t)p * stride];
    size_t at = 0;
    const int m = ms::mark_voxel(Gd, q[0], q[1], q[2], &at);
    if (m > 0) g[at] = 1;
    if (track && m > 0) k[at] = 1;
    stats[3] += m < 0;
  }
  const int32_t has_known = track ? 1 : 0;   // an untracked scan drops the grid
  wr(fo, stats); wr(fo, raw);
  fwrite(&has_known, 4, 1, fo);
  wr(fo, known);
  return 0;
}

// the labelling of free_comp.h on `mask` (k_cc_tile, k_cc_merge, k_cc_flatten, k_cc_sizes as lane loops) -> the error word
static int label_mask(const std::vector<uint8_t>& mask, int X, int Y, int Z, std::vector<int32_t>& parent, std::vector<int32_t>& size,
                      unsigned long long* cnt) {
  const int G = X * Y * Z, tx = (X + 7) / 8, ty = (Y + 7) / 8, tz = (Z + 7) / 8;
  int err = 0;
  for (int t = 0; t < tx * ty * tz; t++) {
    int s_par[fc::kTileVox];
    const int x0 = (t / (ty * tz)) * 8, y0 = ((t / tz) % ty) * 8, z0 = (t % tz) * 8;
    for (int l = 0; l < fc::kTileVox; l++) {
      const int x = x0 + (l >> 6), y = y0 + ((l >> 3) & 7), z = z0 + (l & 7);
      s_par[l] = (x < X && y < Y && z < Z && fc::enterable(mask.data(), nullptr, ((long long)x * Y + y) * Z + z, 0)) ? l : -1;
    }
    auto load = [&](int i) { return s_par[i]; };
    auto amin = [&](int i, int v) { const int old = s_par[i]; if (v < old) s_par[i] = v; return old; };
    for (int l = 0; l < fc::kTileVox; l++) {
      if (s_par[l] < 0) continue;
      for (int k = 0; k < fc::kForward; k++) {
        int dx, dy, dz;
        fc::forward_offset(k, dx, dy, dz);
        const int nx = (l >> 6) + dx, ny = ((l >> 3) & 7) + dy, nz = (l & 7) + dz;
        if (nx >= 8 || ny < 0 || ny >= 8 || nz < 0 || nz >= 8) continue;
        const int m = (nx << 6) | (ny << 3) | nz;
        if (s_par[m] >= 0) fc::unite(load, amin, l, m, fc::kTileVox, &err);
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
  auto load = [&](int i) { return parent[i]; };
  auto amin = [&](int i, int v) { const int old = parent[i]; if (v < old) parent[i] = v; return old; };
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
      if (parent[m] >= 0) fc::unite(load, amin, v, m, G, &err);
    }
  }
  for (int v = 0; v < G; v++) {
    if (parent[v] < 0) continue;
    const int r = fc::root_of(load, v, G, &err);
    parent[v] = r;
    size[r] += 1;
  }
  for (int v = 0; v < G; v++) {
    const int r = parent[v];
    if (r < 0) continue;
    cnt[0]++;
    if (r != v) { size[v] = size[r]; continue; }
    cnt[1]++;
    cnt[2] = std::max(cnt[2], fc::stat_key(size[v], r));
  }
  return err;
}

// op 1, one frontier call.  in: int32 X, Y, Z, min_d2, min_size, capacity; uint8 map[G], known[G]; int32 d2[G] when min_d2 > 1
// out: int64 stats[6], err; int32 label[cap], size[cap], centroid[cap][3], rep[cap][3] (-1 beyond `written`), voxel_label[G]
static int frontier(FILE* fi, FILE* fo) {
  const std::vector<int32_t> h = rd<int32_t>(fi, 6);
  const int X = h[0], Y = h[1], Z = h[2], floor = fc::normal_floor(h[3]), min_size = h[4], G = X * Y * Z;
  const int cap = std::min(h[5], G), nb = (G + 255) / 256;
  const std::vector<uint8_t> map = rd<uint8_t>(fi, G), known = rd<uint8_t>(fi, G);
  const std::vector<int32_t> d2 = rd<int32_t>(fi, floor ? G : 0);
  unsigned long long cnt[4] = {0, 0, 0, 0}, n_known = 0, n_front = 0;
  // ---- k_front_mask
  std::vector<uint8_t> mask(G);
  for (int g = 0; g < G; g++) {
    mask[g] = fr::mask_byte(map.data(), known.data(), floor ? d2.data() : nullptr, g / (Y * Z), (g / Z) % Y, g % Z, X, Y, Z, floor);
    n_known += known[g] != 0;
    n_front += mask[g] == 0;
  }
  std::vector<int32_t> label(G), size(G, 0), slot(G, -7), wg(nb, 0);
  const int err = label_mask(mask, X, Y, Z, label, size, cnt);
  // ---- k_front_count, k_front_scan (64 lanes, a contiguous run each), k_front_scatter
  for (int g = 0; g < G; g++) wg[g / 256] += fr::kept_root(label[g], size[g], g, min_size);
  const int run = (nb + 63) / 64;
  int sums[64], kept = 0;
  for (int lane = 0; lane < 64; lane++) {
    sums[lane] = 0;
    for (int i = std::min(lane * run, nb); i < std::min(lane * run + run, nb); i++) sums[lane] += wg[i];
  }
  for (int lane = 0; lane < 64; lane++) {
    int before = kept;
    kept += sums[lane];
    for (int i = std::min(lane * run, nb); i < std::min(lane * run + run, nb); i++) { const int c = wg[i]; wg[i] = before; before += c; }
  }
  std::vector<int32_t> s_label(cap), s_size(cap);
  std::vector<unsigned long long> s_sum(3 * (size_t)cap, 0), s_key(cap, fr::kNoKey);
  for (int b = 0; b < nb; b++) {
    int pos = 0;
    for (int g = b * 256; g < std::min(G, b * 256 + 256); g++) {
      if (label[g] != g) continue;
      const bool flag = fr::kept_root(label[g], size[g], g, min_size);
      const int s = wg[b] + pos;
      pos += flag;
      slot[g] = flag && s < cap ? s : -1;
      if (slot[g] >= 0) { s_label[s] = g; s_size[s] = size[g]; }
    }
  }
  const int written = std::min(kept, cap);
  auto slot_of = [&](int g) { return g < G && label[g] >= 0 ? slot[label[g]] : -1; };
  // ---- k_front_sum: per wave of 64 voxels and distinct slot, one packed sum
  for (int w = 0; w < nb * 4; w++) {
    bool done[64] = {};
    for (int lead = 0; lead < 64; lead++) {
      const int s0 = slot_of(w * 64 + lead);
      if (s0 < 0 || done[lead]) continue;
      unsigned long long v = 0;
      for (int l = lead; l < 64; l++) {
        const int g = w * 64 + l;
        if (slot_of(g) != s0) continue;
        done[l] = true;
        v += fr::pack_xyz(g / (Y * Z), (g / Z) % Y, g % Z);
      }
      for (int a = 0; a < 3; a++) s_sum[3 * (size_t)s0 + a] += (unsigned long long)fr::packed_axis(v, a);
    }
  }
  // ---- k_front_rep, k_front_unpack
  auto centroid = [&](int s, int32_t* c) { for (int a = 0; a < 3; a++) c[a] = fr::centroid_axis((long long)s_sum[3 * (size_t)s + a], s_size[s]); };
  for (int g = 0; g < G; g++) {
    const int s = slot_of(g);
    if (s < 0) continue;
    int32_t c[3];
    centroid(s, c);
    s_key[s] = std::min(s_key[s], fr::rep_key(g / (Y * Z), (g / Z) % Y, g % Z, c, g));
  }
  std::vector<int32_t> o_label(h[5], -1), o_size(h[5], -1), o_cen(3 * (size_t)h[5], -1), o_rep(3 * (size_t)h[5], -1);
  for (int s = 0; s < written; s++) {
    o_label[s] = s_label[s]; o_size[s] = s_size[s];
    centroid(s, &o_cen[3 * (size_t)s]);
    const int v = fr::key_voxel(s_key[s]);
    o_rep[3 * (size_t)s] = v / (Y * Z); o_rep[3 * (size_t)s + 1] = (v / Z) % Y; o_rep[3 * (size_t)s + 2] = v % Z;
  }
  const std::vector<int64_t> stats = {(int64_t)n_known, (int64_t)n_front, (int64_t)cnt[1], kept, std::min(kept, h[5]), fc::stat_size(cnt[2]), err};
  wr(fo, stats); wr(fo, o_label); wr(fo, o_size); wr(fo, o_cen); wr(fo, o_rep); wr(fo, label);
  return cnt[0] == n_front ? 0 : 4;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 1;
  const int op = rd<int32_t>(fi, 1)[0];
  const int rc = op == 0 ? scan(fi, fo) : frontier(fi, fo);
  fclose(fi);
  fclose(fo);
  return rc;
}
'''


def build(workdir, sanitize=False):
    name = "frontier_harness_san" if sanitize else "frontier_harness"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    return compile_program(workdir, name, HARNESS, extra)


def _exchange(exe, write):
    fin, fout = exe + ".in", exe + ".out"
    with open(fin, "wb") as f:
        write(f)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stderr[-3000:])
    with open(fout, "rb") as f:
        raw = f.read()
    os.remove(fin)
    os.remove(fout)
    return raw


def run_scan(exe, points, origin, max_range, mode=CONTINUE, flags=1, raw=None, known=None, test_store=True, dims=sh.DIMS, res=sh.RES,
             lower=sh.LOWER, upper=sh.UPPER):
    """One scan of the header program on a handle that held the scan grid `raw` (None: empty; the caller passes the map for ADOPT)
    and the known grid `known` (None: none).  -> dict(raw, known or None, stats[4]), or the refusal's number"""
    pts = np.ascontiguousarray(sh.mh._rows(points))
    G = int(np.prod(dims))

    def write(f):
        np.array([0] + list(dims) + [pts.shape[1], mode, flags, int(test_store), int(known is not None)], np.int32).tofile(f)
        np.array([len(pts)], np.int64).tofile(f)
        np.array(list(lower) + list(upper) + [res, max_range] + list(origin), np.float64).tofile(f)
        pts.tofile(f)
        for g in (raw, known):
            (np.zeros(G, np.uint8) if g is None else np.ascontiguousarray(g, np.uint8)).tofile(f)

    out = _exchange(exe, write)
    refused = int(np.frombuffer(out[:4], np.int32)[0])
    if refused:
        assert len(out) == 4
        return refused
    stats = np.frombuffer(out[4:36], np.int64).copy()
    grid = np.frombuffer(out[36:36 + G], np.uint8).reshape(dims).copy()
    has = int(np.frombuffer(out[36 + G:40 + G], np.int32)[0])
    kn = np.frombuffer(out[40 + G:], np.uint8).reshape(dims).copy()
    return dict(raw=grid, known=kn if has else None, stats=stats)


def run_frontier(exe, grid, known, d2=None, min_d2=0, min_size=1, capacity=1024):
    """-> dict(label, size, centroid, rep (the first `written` rows; the rest must be -1), voxel_label, stats[6])"""
    grid = np.ascontiguousarray(grid, np.uint8)
    X, Y, Z = grid.shape
    G = grid.size

    def write(f):
        np.array([1, X, Y, Z, min_d2, min_size, capacity], np.int32).tofile(f)
        grid.tofile(f)
        np.ascontiguousarray(known, np.uint8).tofile(f)
        if min_d2 > 1:
            np.ascontiguousarray(d2, np.int32).tofile(f)

    out = _exchange(exe, write)
    st = np.frombuffer(out[:56], np.int64)
    assert st[6] == 0, "a union-find loop passed its trip bound"
    body = np.frombuffer(out[56:], np.int32)
    assert body.size == 8 * capacity + G
    k, c = int(st[4]), capacity
    parts = dict(label=body[:c], size=body[c:2 * c], centroid=body[2 * c:5 * c].reshape(-1, 3), rep=body[5 * c:8 * c].reshape(-1, 3))
    for key, a in parts.items():
        assert (a[k:] == -1).all(), key
    r = {key: a[:k].copy() for key, a in parts.items()}
    r.update(voxel_label=body[8 * c:].reshape(grid.shape).copy(), stats=st[:6].copy())
    return r
