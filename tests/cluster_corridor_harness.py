"""g++ build of direct_amd/csrc/cluster_corridor_math.h as a program - TEST INFRASTRUCTURE of tests/test_cluster_corridor_cpp.py,
tests/test_gpu_cluster_corridor.py and the stride tests (tests/corridor_stride_lib.py).
The program emulates a whole direct_cluster_corridor_batch call the way the host loop and the kernels of cluster_corridor.h run it:
rounds of advance (every row until it is due or done, with a serial plane test on the double stack), unique (the header's own
serial statement of the de-duplication), chunks of at most `chunk` unique seeds, append, and emit after the last round.  The one
thing it does not compute is a polytope: generation + hull of a seed voxel are looked up in a TABLE keyed by the voxel, which
Python fills from the CPU oracles (oracle.clusterapi.polygon_generation + oracle.hullapi.hull_planes) - so a test can also plant
a failing seed.  A seed that is due and not in the table ends the program with status 3.
This file also holds what the CPU and the GPU tests share: the rows, the oracle's corridors and the comparison."""
import numpy as np

from oracle import clusterapi, corridor_walk, hullapi
from tests import corridor_lib as lib
from tests import cpp_program as cpp
from tests import cube_corridor_harness as ch

OK, OVERFLOW, BAD_PATH, NO_POLYTOPE, TOO_MANY_PLANES = 0, 1, 2, 3, 4
RES, LOWER, DIMS = ch.RES, ch.LOWER, ch.DIMS
CAP, SEG, PMAX = 40, 12, 20          # path_capacity, seg_capacity and p_max of the tests (most planes of a polytope here: 16)
CAPACITY = int(np.prod(DIMS))        # cluster_capacity = candidate_capacity = the map's voxel count: no capacity can be reached
KEYS = ("n_seg", "n_planes", "planes", "seeds", "centers", "rtn")

HARNESS = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include "cluster_corridor_math.h"
namespace kc = direct::clucor;
namespace cc = direct::cubecor;
struct Poly { int gen_ok, hull_rtn, np; std::vector<double> planes; double center[3]; };
template <typename T> static void rd(FILE* f, std::vector<T>& v) { if (v.size() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(1); }
template <typename T> static void wr(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }
static void wr_real(FILE* f, const std::vector<double>& v, int f32) {
  if (!f32) { wr(f, v); return; }
  std::vector<float> w(v.size());
  for (size_t i = 0; i < v.size(); i++) w[i] = (float)v[i];
  wr(f, w);
}
// in: int32 X, Y, Z, n, cap, pop_back, seg_cap, p_max, f32, chunk, n_table, 0; float64 res, lower[3]; int32 path[n][cap][3], len[n];
// then n_table entries of int32 voxel[3], gen_ok, hull_rtn, np; float64 planes[np][4], center[3]
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[12];
  double g[4];
  if (!f || fread(h, 4, 12, f) != 12 || fread(g, 8, 4, f) != 4) return 1;
  const int X = h[0], Y = h[1], Z = h[2], n = h[3], cap = h[4], pop_back = h[5], S = h[6], P = h[7], f32 = h[8], chunk = h[9], n_table = h[10];
  const double res = g[0], *lower = g + 1;
  std::vector<int32_t> path(3 * (size_t)n * cap), len(n);
  rd(f, path); rd(f, len);
  std::map<int, Poly> table;
  for (int i = 0; i < n_table; i++) {
    std::vector<int32_t> e(6);
    rd(f, e);
    Poly p;
    p.gen_ok = e[3]; p.hull_rtn = e[4]; p.np = e[5];
    p.planes.resize(4 * (size_t)p.np);
    rd(f, p.planes);
    if (fread(p.center, 8, 3, f) != 3) return 1;
    table[kc::voxel_index(e.data(), Y, Z)] = p;
  }
  fclose(f);
  // the workspace of the call
  std::vector<kc::Row> rows(n);
  std::vector<double> st_planes(4 * (size_t)n * S * P, -7.0), st_seeds(3 * (size_t)n * S, -7.0), st_centers(3 * (size_t)n * S, -7.0);  // dirty on purpose
  std::vector<int32_t> st_np((size_t)n * S, 99), seed_list(3 * (size_t)n);
  std::vector<int> owner((size_t)X * Y * Z, kc::kNoOwner);
  std::vector<double> h_planes(4 * (size_t)chunk * P), h_center(3 * (size_t)chunk);
  std::vector<int32_t> h_np(chunk), h_rtn(chunk), h_gen(chunk);
  long long stats[4] = {0, 0, 0, 0};
  bool ended = false;
  for (int round = 0; round <= cap && !ended; round++) {
    for (int b = 0; b < n; b++) {  // k_corr_advance
      const int32_t* p = &path[3 * (size_t)b * cap];
      if (round == 0) {
        bool bad = len[b] <= 0 || len[b] > cap;
        for (int i = 0; !bad && i < len[b]; i++) bad = !kc::voxel_inside(p + 3 * i, X, Y, Z);
        rows[b] = kc::row_start(bad);
      }
      if (rows[b].state != kc::kWalking) continue;
      const int pops = rows[b].pops;
      kc::advance(rows[b], p, len[b], S, pop_back, res, lower, [&](int level, const double* cur) {
        const size_t at = (size_t)b * S + level;
        for (int t = 0; t < st_np[at]; t++)
          if (cc::plane_excludes(cur, &st_planes[(at * P + t) * 4])) return true;
        return false;
      });
      stats[3] += rows[b].pops - pops;
    }
    int due = 0;
    const int uniq = kc::unique_seeds(rows.data(), n, Y, Z, owner.data(), seed_list.data(), &due);  // k_corr_unique
    for (int v : owner) if (v != kc::kNoOwner) return 4;
    stats[1] += due; stats[2] += uniq;
    if (uniq == 0) { ended = true; break; }
    stats[0]++;
    for (int lo = 0; lo < uniq; lo += chunk) {
      const int nb = uniq - lo < chunk ? uniq - lo : chunk;
      for (int j = 0; j < nb; j++) {  // generation + hull with a plane capacity of P, as k_hull_finish reports it
        auto it = table.find(kc::voxel_index(&seed_list[3 * (lo + j)], Y, Z));
        if (it == table.end()) return 3;
        const Poly& q = it->second;
        h_gen[j] = q.gen_ok;
        h_np[j] = q.hull_rtn == kc::kHullOk ? q.np : 0;
        h_rtn[j] = (q.hull_rtn == kc::kHullOk && q.np > P) ? kc::kHullOverflow : q.hull_rtn;
        for (int t = 0; t < 4 * q.np && t < 4 * P; t++) h_planes[4 * (size_t)j * P + t] = q.planes[t];
        for (int a = 0; a < 3; a++) h_center[3 * j + a] = q.center[a];
      }
      for (int b = 0; b < n; b++) {  // k_corr_append
        kc::Row& r = rows[b];
        if (r.state != kc::kDue || r.slot < lo || r.slot >= lo + nb) continue;
        const int j = r.slot - lo;
        const int code = kc::judge(h_gen[j] != 0, h_rtn[j], h_np[j], P);
        if (code != kc::kOk) { kc::stop(r, code); continue; }
        const size_t at = (size_t)b * S + r.depth;
        for (int t = 0; t < 4 * h_np[j]; t++) st_planes[at * P * 4 + t] = h_planes[4 * (size_t)j * P + t];
        st_np[at] = h_np[j];
        cc::index2coord(r.seed, res, lower, &st_seeds[3 * at]);
        for (int a = 0; a < 3; a++) st_centers[3 * at + a] = h_center[3 * j + a];
        kc::push(r);
      }
    }
  }
  if (!ended) return 5;
  // k_corr_emit
  std::vector<int32_t> n_seg(n), n_planes((size_t)n * S), rtn(n);
  std::vector<double> planes(4 * (size_t)n * S * P), seeds(3 * (size_t)n * S), ctrs(3 * (size_t)n * S);
  for (int b = 0; b < n; b++) {
    const kc::Row& r = rows[b];
    const size_t seg0 = (size_t)b * S;
    n_seg[b] = r.depth; rtn[b] = r.code;
    for (int k = 0; k < S; k++) {
      n_planes[seg0 + k] = k < r.depth ? st_np[seg0 + k] : 0;
      for (int a = 0; a < 3; a++) {
        seeds[3 * (seg0 + k) + a] = k < r.depth ? st_seeds[3 * (seg0 + k) + a] : 0.0;
        ctrs[3 * (seg0 + k) + a] = k < r.depth ? st_centers[3 * (seg0 + k) + a] : 0.0;
      }
    }
    for (int q = 0; q < S * P * 4; q++) planes[seg0 * P * 4 + q] = kc::emit_plane(r, &st_planes[seg0 * P * 4], &st_np[seg0], P, q);
  }
  FILE* o = fopen(argv[2], "wb");
  wr(o, n_seg); wr(o, n_planes); wr_real(o, planes, f32); wr_real(o, seeds, f32); wr_real(o, ctrs, f32); wr(o, rtn);
  fwrite(stats, 8, 4, o);
  fclose(o);
  return 0;
}
'''


def build(workdir):
    return str(workdir), cpp.compile_program(workdir, "cluster_corridor_harness", HARNESS, ["-Wno-unknown-pragmas"])


def corridors(harness, paths, path_len, table, pop_back=True, seg_capacity=SEG, p_max=PMAX, dtype=np.float64, chunk=64, res=RES, lower=LOWER,
              dims=DIMS):
    """the outputs of ClusterGenerator.cluster_corridors for the same arguments on a handle with max_batch = chunk, polytopes from
    `table`: voxel (x, y, z) -> dict(gen_ok, rc, n_planes, planes [n][4], center [3])"""
    paths, path_len = np.ascontiguousarray(paths, np.int32), np.ascontiguousarray(path_len, np.int32)
    B, cap = paths.shape[0], paths.shape[1]
    S, P, real = int(seg_capacity), int(p_max), np.dtype(dtype)
    arrays = [paths, path_len]
    for key, t in table.items():
        pl = np.ascontiguousarray(t["planes"], np.float64).reshape(-1, 4)
        arrays += [np.array(list(key) + [int(t["gen_ok"]), int(t["rc"]), len(pl)], np.int32), pl, np.asarray(t["center"], np.float64)]
    raw = cpp.exchange(harness, list(dims) + [B, cap, int(pop_back), S, P, int(real == np.float32), int(chunk), len(table), 0],
                       [res] + list(lower), arrays)
    out = cpp.unpack(raw, (("n_seg", np.int32, (B,)), ("n_planes", np.int32, (B, S)), ("planes", real, (B, S, P, 4)), ("seeds", real, (B, S, 3)),
                           ("centers", real, (B, S, 3)), ("rtn", np.int32, (B,)), ("stats", np.int64, (4,))))
    out["stats"] = dict(zip(("rounds", "due_seeds", "unique_seeds", "pops"), (int(v) for v in out["stats"])))
    return out


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------

def inside_rows():
    """the paths of the named cases that lie inside the map, and eight random walks: the first 23 of the 40 rows"""
    rows = lib.named_rows() + ch.random_paths(ch.crafted_map(), 8, seed=9)
    assert len(rows) == 23 and all(np.array_equal(a, b) for a, b in zip(rows, lib.rows40()))
    return rows


def shared_start_rows():
    """six paths that all start at [5, 5, 5]: the first polytope of every row is the same seed"""
    ends = ([7, 7, 7], [3, 3, 3], [7, 3, 5], [5, 7, 3], [3, 5, 7], [8, 5, 5])
    return [np.asarray(ch.line([5, 5, 5], e), np.int32) for e in ends]


_ORACLE = {}


def oracle_corridors(rows, itr_cluster_max, pop_back, grid=None, tag="crafted"):
    """oracle.corridor_walk for every row (voxel centres in, so its snap returns the voxel) with one cache of polytopes per
    (map, itr_cluster_max), computed once per process -> (list of (corridor, ok), table for corridors())"""
    grid = ch.crafted_map() if grid is None else grid
    cache = _ORACLE.setdefault((tag, itr_cluster_max), {})
    out = []
    for p in rows:
        coords = np.asarray(p, np.float64) * RES + 0.5 * RES + LOWER
        cor, ok = corridor_walk.corridor_generation(grid, RES, LOWER, coords, 1000, itr_cluster_max, cache, pop=pop_back)
        out.append((cor, ok))
    table = {k: dict(gen_ok=1, rc=r["rc"], planes=r["planes"], center=r["center"]) for k, r in cache.items()}
    return out, table


def polytope(grid, voxel, itr_cluster_max):
    """one table entry from the CPU oracles"""
    r = hullapi.hull_planes(clusterapi.polygon_generation(grid, tuple(int(v) for v in voxel), 1000, itr_cluster_max)[1], RES, LOWER)
    return dict(gen_ok=1, rc=r["rc"], planes=r["planes"], center=r["center"])


def assert_rows_equal_oracle(got, want, rows):
    """n_seg, n_planes, planes, seeds and centres of every row against the oracle's corridor, to the bit, zeros behind"""
    for b, (cor, ok) in enumerate(want):
        k = len(cor)
        assert ok and got["rtn"][b] == OK and got["n_seg"][b] == k, (b, got["rtn"][b], got["n_seg"][b], k)
        assert got["n_planes"][b, :k].tolist() == [len(c["planes"]) for c in cor], b
        for s, c in enumerate(cor):
            n = len(c["planes"])
            assert np.array_equal(got["planes"][b, s, :n], c["planes"]) and not got["planes"][b, s, n:].any(), (b, s)
            assert np.array_equal(got["centers"][b, s], c["center"]) and np.array_equal(got["seeds"][b, s], c["seed_coord"]), (b, s)
        for key in ("n_planes", "planes", "seeds", "centers"):
            assert not got[key][b, k:].any(), (b, key)
