"""TEST INFRASTRUCTURE of tests/test_plan_check_restatement.py, tests/test_gpu_plan_check.py and tools/plan_check_bench.py: what
direct_cluster_plan_check_batch (include/direct_cluster.h, "plans against the resident map") must return, twice over.
  restate      NumPy, written from the header's text, NOT from direct_amd/csrc/plan_check_math.h: it forms ALL 2^D leaves of every
               segment by halving, judges every one of them and takes the first blocked judged one.  Occupancy is read from the
               map itself (a slice), not from a summed-area table.
  build / run  a g++ -O2 -ffp-contract=off program around plan_check_math.h that runs the header's pruned DESCENT on one thread,
               with a summed-area table of its own; it also checks the nesting of every visited parent / child pair, counts its
               box tests and times itself (for the bench tool).
  dyadic       the curve's points at the dyadic parameters of a depth, by the same halving: the soundness test's samples.
  plan_rows / ROW_FRONT / row_section   the row front of the restatements (NumPy) and of the programs (C++, with the writer of
               what it reads), each kept once here for tests/dist_field_harness.py too: validity, start times, control points.
and the inputs the CPU and the GPU tests share."""
import os
import subprocess

import numpy as np

from tests.cpp_program import compile_program
from tests.map_cloud_harness import DIMS, LOWER, RES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
MAX_COORD = 1e300
BINOM = np.array([[1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 2, 1, 0, 0, 0], [1, 3, 3, 1, 0, 0], [1, 4, 6, 4, 1, 0],
                  [1, 5, 10, 10, 5, 1]], np.float64)


# ---- the restatement -------------------------------------------------------------------------------------------------

def control_points(coef, T, poly):
    """item 1: [3][6] control points in metres of one segment from its 18 stored numbers (already double)"""
    c = np.asarray(coef, np.float64)
    T = np.float64(T)
    with np.errstate(all="ignore"):
        if not poly:
            return T * c.reshape(3, 6)
        a = c.reshape(6, 3)
        Tm = [np.float64(1.0)]
        for m in range(1, 6):
            Tm.append(Tm[-1] * T)
        P = np.zeros((3, 6))
        for d in range(3):
            s = [a[m, d] * Tm[m] for m in range(6)]
            for j in range(6):
                b = None
                for m in range(j + 1):
                    t = (BINOM[j, m] / BINOM[5, m]) * s[m]
                    b = t if b is None else b + t
                P[d, j] = b
        return P


def halve_all(P):
    """[n][3][6] -> [2n][3][6]: child 2k is the left half of k, child 2k + 1 the right; every new point is (a + b) * 0.5"""
    w = P.copy()
    L, R = np.empty_like(P), np.empty_like(P)
    L[..., 0], R[..., 5] = w[..., 0], w[..., 5]
    for lvl in range(1, 6):
        w = (w[..., :-1] + w[..., 1:]) * 0.5
        L[..., lvl], R[..., 5 - lvl] = w[..., 0], w[..., -1]
    out = np.empty((2 * len(P),) + P.shape[1:])
    out[0::2], out[1::2] = L, R
    return out


def leaves(P, depth):
    out = np.asarray(P, np.float64)[None]
    for _ in range(depth):
        out = halve_all(out)
    return out


def index_box(P, lower, inv, margin, dims):
    """item 3 for [n][3][6] point sets -> lo [n][3], hi [n][3]"""
    size = np.asarray(dims, np.float64)
    with np.errstate(all="ignore"):
        qlo = ((P.min(axis=2) - margin) - lower) * inv
        qhi = ((P.max(axis=2) + margin) - lower) * inv

        def vox(q):
            t = np.trunc(np.where((q >= 0) & (q < size), q, 0.0)).astype(np.int64)
            return np.where(q >= size, np.asarray(dims), np.where(~(q >= 0), -1, t))
        return vox(qlo), vox(qhi)


def box_flags(lo, hi, grid):
    """-> occupied | leaves << 1 for one box"""
    dims = grid.shape
    leaves_map = bool((lo == -1).any() or (hi == np.asarray(dims)).any())
    clo, chi = np.maximum(lo, 0), np.minimum(hi, np.asarray(dims) - 1)
    occ = bool((clo <= chi).all()) and bool((grid[clo[0]:chi[0] + 1, clo[1]:chi[1] + 1, clo[2]:chi[2] + 1] == 1).any())
    return int(occ) | (int(leaves_map) << 1)


def starts(Trow, n):
    return np.concatenate([[0.0], np.cumsum(np.asarray(Trow[:n], np.float64))])


def plan_rows(inp, use_t_from=True):
    """The front of both restatements (this one and dist_field_harness.restate_clearance).  inp: dict(n_seg [B], T [B][N], bez or
    poly [B][N][18], t_from [B] or absent); float32 inputs are promoted exactly, as the kernels do.
    -> (T [B][N] float64, t_from [B] or None, rows): rows[b] = (n_seg, whether the row is valid, and for a valid row its control
    points in metres [n][3][6] and its start times S [n + 1])"""
    n_seg = np.asarray(inp["n_seg"], np.int32)
    T = np.asarray(inp["T"]).astype(np.float64)
    poly = inp.get("poly") is not None
    coef = np.asarray(inp["poly"] if poly else inp["bez"]).astype(np.float64)
    t_from = inp.get("t_from") if use_t_from else None
    B, N = T.shape
    rows = []
    for b in range(B):
        n = int(n_seg[b])
        ok = 1 <= n <= N and bool(np.all(np.isfinite(T[b, :n]) & (T[b, :n] > 0)))
        ok = ok and not (t_from is not None and np.isnan(t_from[b]))
        pts = [control_points(coef[b, i], T[b, i], poly) for i in range(n)] if ok else []
        ok = ok and all(bool(np.all(np.abs(p) <= MAX_COORD)) for p in pts)  # False for NaN
        rows.append((n, ok, pts, starts(T[b], n) if ok else None))
    return T, t_from, rows


def restate(inp, grid, depth, margin=0.0, outside_blocks=False, use_t_from=True, lower=LOWER, res=RES):
    """inp as plan_rows takes it -> dict of the call's outputs as they read in HOST memory"""
    T, t_from, rows = plan_rows(inp, use_t_from)
    B, N = T.shape
    inv = 1.0 / res
    lower = np.asarray(lower, np.float64)
    out = dict(status=np.zeros(B, np.int32), verdict=np.zeros(B, np.int32), t_free=np.zeros(B), first=np.full((B, 2), -1, np.int32),
               hit_box=np.full((B, 6), -1, np.int32), seg_first=np.full((B, N), -1, np.int32))
    for b, (n, ok, pts, S) in enumerate(rows):
        if not ok:
            out["status"][b], out["verdict"][b] = -1, INVALID
            continue
        out["t_free"][b] = S[n]
        for i in range(n):
            L = leaves(pts[i], depth)
            k = np.arange(1 << depth, dtype=np.float64)
            t0 = S[i] + (k * 2.0 ** -depth) * T[b, i]
            t1 = S[i] + ((k + 1) * 2.0 ** -depth) * T[b, i]
            judged = np.ones(len(k), bool) if t_from is None else t1 > t_from[b]
            lo, hi = index_box(L, lower, inv, margin, grid.shape)
            boxes, which = np.unique(np.concatenate([lo, hi], axis=1), axis=0, return_inverse=True)   # deep leaves share boxes
            flags = np.array([box_flags(u[:3], u[3:], grid) for u in boxes])[which.reshape(-1)]
            blocked = judged & (((flags & 1) != 0) | (bool(outside_blocks) & ((flags & 2) != 0)))
            if blocked.any():
                kk = int(np.argmax(blocked))
                out["seg_first"][b, i] = kk
                if out["first"][b, 0] < 0:
                    out["first"][b] = (i, kk)
                    out["verdict"][b], out["t_free"][b] = flags[kk], t0[kk]
                    out["hit_box"][b] = np.concatenate([lo[kk], hi[kk]])
    return out


def dyadic(inp, b, depth):
    """-> (times [m], points [m][3]) of row b at the dyadic parameters of `depth` in every segment, by halving"""
    poly = inp.get("poly") is not None
    coef = np.asarray(inp["poly"] if poly else inp["bez"]).astype(np.float64)
    T = np.asarray(inp["T"]).astype(np.float64)
    n = int(inp["n_seg"][b])
    S = starts(T[b], n)
    ts, ps = [], []
    for i in range(n):
        L = leaves(control_points(coef[b, i], T[b, i], poly), depth)
        k = np.arange((1 << depth) + 1, dtype=np.float64)
        ts.append(S[i] + (k * 2.0 ** -depth) * T[b, i])
        ps.append(np.concatenate([L[:, :, 0], L[-1:, :, 5]]))
    return np.concatenate(ts), np.concatenate(ps)


def voxel_bytes(points, grid, lower=LOWER, res=RES):
    """the map byte of every point's voxel (0 for a point outside the map)"""
    q = (np.asarray(points) - np.asarray(lower)) * (1.0 / res)
    inside = ((q >= 0) & (q < np.asarray(grid.shape))).all(axis=1)
    idx = np.trunc(np.where(inside[:, None], q, 0.0)).astype(np.int64)
    return np.where(inside, grid[idx[:, 0], idx[:, 1], idx[:, 2]], 0)


# ---- the header's descent, compiled by g++ -----------------------------------------------------------------------------

# The row front of this module's program and of dist_field_harness's: the row section of an input file (row_section() writes it),
# per row its validity, start times and control points, and the grid fields both headers' Grids have.  The start-time rule is
# stated here on its own (a sum left to right, every T > 0 and finite), NOT taken from traj_eval_math.h, which the kernels use.
ROW_FRONT = r'''
namespace pk = direct::plancheck;
struct Rows {
  int B, N, poly, has_from;
  std::vector<int> n_seg;
  std::vector<double> T, coef, t_from;
};
// int32 n_seg[B]; float64 T[B][N], coef[B][N][18], t_from[B] (when has_from)
static bool read_rows(FILE* f, Rows& R) {
  const size_t B = R.B, slots = B * R.N;
  R.n_seg.resize(B); R.T.resize(slots); R.coef.resize(slots * 18); R.t_from.assign(B, 0.0);
  return fread(R.n_seg.data(), 4, B, f) == B && fread(R.T.data(), 8, slots, f) == slots &&
         fread(R.coef.data(), 8, slots * 18, f) == slots * 18 && (!R.has_from || fread(R.t_from.data(), 8, B, f) == B);
}
// whether row b is valid; then S[0 .. n] and the control points P[i * 18 ..] of its n segments
static int row_front(const Rows& R, int b, std::vector<double>& S, std::vector<double>& P) {
  const int n = R.n_seg[b];
  const double* T = &R.T[(size_t)b * R.N];
  int ok = 1 <= n && n <= R.N;
  if (ok) {
    S[0] = 0.0;
    for (int i = 0; i < n; i++) {
      ok &= (T[i] > 0.0 && T[i] <= 1.7976931348623157e308) ? 1 : 0;
      S[i + 1] = S[i] + T[i];
    }
  }
  if (R.has_from && R.t_from[b] != R.t_from[b]) ok = 0;
  P.resize((size_t)(ok ? n : 0) * 18);  // reused from row to row: every entry a caller reads is written below
  for (int i = 0; ok && i < n; i++) {
    const double* c = &R.coef[((size_t)b * R.N + i) * 18];
    ok &= R.poly ? pk::ctrl_from_poly(c, T[i], &P[i * 18]) : pk::ctrl_from_bez(c, T[i], &P[i * 18]);
  }
  return ok;
}
template <class Grid>
static void grid_front(Grid& g, const double* lower, double res, int X, int Y, int Z) {
  for (int a = 0; a < 3; a++) g.lower[a] = lower[a];
  g.inv = 1.0 / res;
  g.size[0] = X; g.size[1] = Y; g.size[2] = Z;
}
'''

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "plan_check_math.h"
''' + ROW_FRONT + r'''
// in: int32 B, N, poly, D, outside, has_from, X, Y, Z, reps, pad, pad; float64 lower[3], res, margin; the row section;
//     uint8 map[G]
// out: int32 status[B], verdict[B], first[B][2], hit_box[B][6], seg_first[B][N]; float64 t_free[B];
//      int64 box tests, parent/child pairs, pairs not nested, 0; float64 ms (best of reps)
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[12];
  double d[5];
  if (!f || fread(h, 4, 12, f) != 12 || fread(d, 8, 5, f) != 5) return 1;
  const int B = h[0], N = h[1], D = h[3], has_from = h[5], X = h[6], Y = h[7], Z = h[8], reps = h[9];
  const size_t G = (size_t)X * Y * Z;
  Rows R = {B, N, h[2], has_from};
  std::vector<uint8_t> map(G);
  if (!read_rows(f, R) || fread(map.data(), 1, G, f) != G) return 1;
  fclose(f);
  pk::Grid grid;
  grid_front(grid, d, d[3], X, Y, Z);
  grid.margin = d[4];
  grid.outside_blocks = h[4];
  // obstacles in [0, x) x [0, y) x [0, z)
  const int sz = Z + 1, syz = (Y + 1) * sz;
  std::vector<int> sat((size_t)(X + 1) * syz, 0);
  for (int x = 1; x <= X; x++)
    for (int y = 1; y <= Y; y++)
      for (int z = 1; z <= Z; z++)
        sat[x * syz + y * sz + z] = (map[((size_t)(x - 1) * Y + (y - 1)) * Z + (z - 1)] == 1) + sat[(x - 1) * syz + y * sz + z] +
                                    sat[x * syz + (y - 1) * sz + z] + sat[x * syz + y * sz + z - 1] - sat[(x - 1) * syz + (y - 1) * sz + z] -
                                    sat[(x - 1) * syz + y * sz + z - 1] - sat[x * syz + (y - 1) * sz + z - 1] +
                                    sat[(x - 1) * syz + (y - 1) * sz + z - 1];
  auto occupied = [&](const int* lo, const int* hi) {
    auto at = [&](int x, int y, int z) { return sat[x * syz + y * sz + z]; };
    const int x0 = lo[0], y0 = lo[1], z0 = lo[2], x1 = hi[0] + 1, y1 = hi[1] + 1, z1 = hi[2] + 1;
    return at(x1, y1, z1) - at(x0, y1, z1) - at(x1, y0, z1) - at(x1, y1, z0) + at(x0, y0, z1) + at(x0, y1, z0) + at(x1, y0, z0) -
               at(x0, y0, z0) > 0;
  };
  std::vector<int> status(B), verdict(B), first((size_t)B * 2), hit((size_t)B * 6), seg_first((size_t)B * N);
  std::vector<double> t_free(B), S(N + 1), P;
  long long extra[4] = {0, 0, 0, 0};
  int path_k[pk::kMaxDepth + 1], path_box[pk::kMaxDepth + 1][6];
  auto visit = [&](int dd, int k, const int* lo, const int* hi, int) {
    if (dd > 0) {
      extra[1]++;
      bool in = path_k[dd - 1] == (k >> 1);
      for (int a = 0; a < 3; a++) in = in && lo[a] >= path_box[dd - 1][a] && hi[a] <= path_box[dd - 1][3 + a] && lo[a] <= hi[a];
      if (!in) extra[2]++;
    }
    path_k[dd] = k;
    for (int a = 0; a < 3; a++) { path_box[dd][a] = lo[a]; path_box[dd][3 + a] = hi[a]; }
  };
  double best = 1e300;
  for (int rep = 0; rep < reps; rep++) {
    extra[0] = extra[1] = extra[2] = 0;
    const auto c0 = std::chrono::steady_clock::now();
    for (int b = 0; b < B; b++) {
      const int n = R.n_seg[b];
      for (int i = 0; i < N; i++) seg_first[(size_t)b * N + i] = -1;
      for (int q = 0; q < 2; q++) first[b * 2 + q] = -1;
      for (int q = 0; q < 6; q++) hit[b * 6 + q] = -1;
      const int ok = row_front(R, b, S, P);
      status[b] = ok ? 0 : -1;
      verdict[b] = ok ? 0 : -1;
      t_free[b] = ok ? S[n] : 0.0;
      for (int i = 0; ok && i < n; i++) {
        const double Ti = R.T[(size_t)b * N + i];
        const int k = pk::descend(&P[i * 18], S[i], Ti, D, 0, 0, has_from, R.t_from[b], grid, occupied, visit, -1, &extra[0]);
        seg_first[(size_t)b * N + i] = k;
        if (k >= 0 && first[b * 2] < 0) {
          double leaf[18];
          int lo[3], hi[3], blocked;
          pk::derive(&P[i * 18], D, k, leaf);
          verdict[b] = pk::judge(leaf, grid, occupied, lo, hi, &blocked);
          first[b * 2] = i; first[b * 2 + 1] = k;
          for (int a = 0; a < 3; a++) { hit[b * 6 + a] = lo[a]; hit[b * 6 + 3 + a] = hi[a]; }
          t_free[b] = pk::node_time(S[i], Ti, D, k);
        }
      }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
    if (ms < best) best = ms;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 1;
  fwrite(status.data(), 4, B, o);
  fwrite(verdict.data(), 4, B, o);
  fwrite(first.data(), 4, first.size(), o);
  fwrite(hit.data(), 4, hit.size(), o);
  fwrite(seg_first.data(), 4, seg_first.size(), o);
  fwrite(t_free.data(), 8, B, o);
  fwrite(extra, 8, 4, o);
  fwrite(&best, 8, 1, o);
  fclose(o);
  return 0;
}
'''


def build(workdir):
    return str(workdir), compile_program(workdir, "plan_check_harness", HARNESS)


def row_section(inp, use_t_from=True):
    """-> ([B, N, poly, has_from], the bytes of the row section of a harness input file): what ROW_FRONT's read_rows reads"""
    poly = inp.get("poly") is not None
    T = np.asarray(inp["T"]).astype(np.float64)
    t_from = inp.get("t_from") if use_t_from else None
    parts = [np.asarray(inp["n_seg"], np.int32), T, np.asarray(inp["poly"] if poly else inp["bez"]).astype(np.float64)]
    parts += [] if t_from is None else [np.asarray(t_from, np.float64)]
    return list(T.shape) + [int(poly), int(t_from is not None)], b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def run(harness, inp, grid, depth, margin=0.0, outside_blocks=False, use_t_from=True, lower=LOWER, res=RES, reps=1):
    """-> (outputs as restate() gives them, dict(tests, pairs, not_nested, ms)) of the header's descent"""
    d, exe = harness
    (B, N, poly, has_from), rows = row_section(inp, use_t_from)
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([B, N, poly, depth, int(outside_blocks), has_from] + list(grid.shape) + [reps, 0, 0], np.int32).tobytes())
        f.write(np.array(list(lower) + [res, margin], np.float64).tobytes() + rows + np.ascontiguousarray(grid, np.uint8).tobytes())
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        out = dict(status=np.fromfile(f, np.int32, B), verdict=np.fromfile(f, np.int32, B), first=np.fromfile(f, np.int32, B * 2).reshape(B, 2),
                   hit_box=np.fromfile(f, np.int32, B * 6).reshape(B, 6), seg_first=np.fromfile(f, np.int32, B * N).reshape(B, N),
                   t_free=np.fromfile(f, np.float64, B))
        extra = np.fromfile(f, np.int64, 4)
        ms = float(np.fromfile(f, np.float64, 1)[0])
        assert f.read() == b""
    os.remove(fout)
    return out, dict(tests=int(extra[0]), pairs=int(extra[1]), not_nested=int(extra[2]), ms=ms)


KEYS = ("status", "verdict", "first", "hit_box", "seg_first", "t_free")


def assert_same(got, want, what=""):
    """every integer and every bit of t_free"""
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "t_free":
            g, w = g.astype(np.float64).view(np.uint64), w.astype(np.float64).view(np.uint64)
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {k} differs\n{got[k]}\n{want[k]}"


# ---- the inputs the CPU and the GPU tests share --------------------------------------------------------------------------
# The map of tests/map_cloud_harness.py (40 x 36 x 12 voxels of 0.15 m).  Its right half (x index >= 20) holds random obstacle blocks;
# the left half holds the few voxels the crafted rows are built around, on "lanes" along x: lane l runs at y index 3 l + 1,
# z index 6 (blocks span z 5..7), three voxels from the next lane, so that a margin of 0.2 m never reaches a neighbour's blocks.

def lane_y(l):
    return LOWER[1] + RES * (3 * l + 1) + 0.07


LANE_Z = 0.97          # z index 6
DIAG_Z = 1.55          # z index 10: the conservative row's own layer


def shared_map(seed=3, blocks=60):
    grid = np.zeros(DIMS, np.uint8)
    rng = np.random.default_rng(seed)
    for _ in range(blocks):
        lo = np.array([rng.integers(20, DIMS[0] - 1), rng.integers(0, DIMS[1] - 1), rng.integers(0, DIMS[2] - 1)])
        ext = rng.integers(1, 5, 3)
        grid[lo[0]:lo[0] + ext[0], lo[1]:lo[1] + ext[1], lo[2]:lo[2] + ext[2]] = 1

    def lane_block(l, ix, dy=0):
        grid[ix, 3 * l + 1 + dy, 5:8] = 1
    lane_block(1, 0)               # leaf0: the voxel of the row's first point
    lane_block(2, 11)              # lastleaf: x in [-1.35, -1.2)
    lane_block(3, 14); lane_block(3, 15)   # later: x in [-0.9, -0.6), the row's third segment
    lane_block(4, 4); lane_block(4, 14)    # from_later: one block in segment 0, one in segment 2
    lane_block(5, 4)               # from_free: one block in segment 0
    lane_block(9, 8, dy=1)         # margin: beside the lane, not on it
    grid[1, 11, 10] = 1            # conservative: the voxel the diagonal's boxes touch and the line never enters
    return grid


def _line(A, B):
    """control points in metres [3][6] of the straight segment A -> B"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return (A[:, None] + (B - A)[:, None] * (np.arange(6) / 5.0)[None, :])


def to_bez(P, T):
    """getBezCoeff() layout [18] of control points in metres: c_j = P_j / T"""
    return (np.asarray(P, np.float64) / T).reshape(18)


def to_poly(P, T):
    """getPolyCoeff() layout [18]: a_m = C(5, m) Delta^m P_0 / T^m"""
    P = np.asarray(P, np.float64)
    a = np.zeros((6, 3))
    w = P.copy()
    for m in range(6):
        a[m] = BINOM[5, m] * w[:, 0] / T ** m
        w = w[:, 1:] - w[:, :-1]
    return a.reshape(18)


def pack(rows, n_max, t_from=None):
    """rows: list of lists of ([3][6] control points in metres, T) -> input dict with both bez and poly of the same curves"""
    B = len(rows)
    n_seg = np.array([len(r) for r in rows], np.int32)
    T, bez, poly = np.ones((B, n_max)), np.zeros((B, n_max, 18)), np.zeros((B, n_max, 18))
    for b, r in enumerate(rows):
        for i, (P, Ti) in enumerate(r[:n_max]):
            T[b, i], bez[b, i], poly[b, i] = Ti, to_bez(P, Ti), to_poly(P, Ti)
    out = dict(n_seg=n_seg, T=T, bez=bez, poly=poly)
    if t_from is not None:
        out["t_from"] = np.asarray(t_from, np.float64)
    return out


def pick(inp, kind):
    """the input with only one of bez / poly"""
    out = {k: v for k, v in inp.items() if k not in ("bez", "poly")}
    out[kind] = inp[kind]
    return out


def as_f32(inp):
    """what a float32 caller stores: T and the coefficients rounded to float32 (t_from stays double)"""
    return {k: (np.asarray(v, np.float32) if k in ("T", "bez", "poly") else v) for k, v in inp.items()}


CRAFTED = ("free", "leaf0", "lastleaf", "later", "from_later", "from_free", "leaving", "outside", "conservative", "margin")
CRAFTED_DEPTH = 5        # the depth the rows' names are true at ("conservative": depth 2)


def crafted_rows():
    """straight rows, T = 1 per segment; see shared_map for the voxels they meet"""
    def lane(l, xs):
        return [(_line([xs[i], lane_y(l), LANE_Z], [xs[i + 1], lane_y(l), LANE_Z]), 1.0) for i in range(len(xs) - 1)]
    three = [-2.9, -2.1, -1.3, -0.5]
    rows = dict(
        free=lane(0, three[:3]),
        leaf0=lane(1, three[:3]),
        lastleaf=lane(2, [-2.92, -1.32]),           # leaf 31 of 32 is x in [-1.37, -1.32], leaf 30 ends at -1.37 < -1.35
        later=lane(3, three),
        from_later=lane(4, three),
        from_free=lane(5, three),
        leaving=lane(6, [-2.9, -3.3, -3.9]),        # crosses the map's lower x face, then runs outside
        outside=lane(7, [-3.5, -3.2]),              # never inside
        # y = x + 2: crosses the y face -0.9 at x = -2.9 and the x face at -2.85, so it passes voxels (0, 11), (0, 12), (1, 12) and
        # never (1, 11); leaf 0 of depth 2 spans x in [-2.93, -2.78] and its box holds all four
        conservative=[(_line([-2.93, -0.93, DIAG_Z], [-2.33, -0.33, DIAG_Z]), 1.0)],
        margin=lane(9, three[:3]),
    )
    return [rows[k] for k in CRAFTED]


def crafted():
    """batch 10, n_seg_max 5; t_from = 1.0 (the start of segment 1) for the two from_ rows, -inf elsewhere"""
    t_from = np.array([1.0 if k.startswith("from_") else -np.inf for k in CRAFTED])
    return pack(crafted_rows(), 5, t_from)


def random_rows(batch, n_max, seed, n_seg=None):
    """random quintics: a random walk of control points through the map, C0 at the joints, durations in [0.5, 2]"""
    rng = np.random.default_rng(seed)
    size = np.array(DIMS) * RES
    rows = []
    for b in range(batch):
        n = int(rng.integers(1, n_max + 1)) if n_seg is None else int(n_seg[b])
        p = LOWER + (np.array([0.3, 0.1, 0.2]) + np.array([0.6, 0.8, 0.6]) * rng.random(3)) * size
        row = []
        for _ in range(n):
            step = rng.normal(0.0, 0.25, (3, 6)) * np.array([1.0, 1.0, 0.3])[:, None]
            step[:, 0] = 0.0
            P = p[:, None] + np.cumsum(step, axis=1)
            row.append((P, float(0.5 + 1.5 * rng.random())))
            p = P[:, 5]
        rows.append(row)
    return rows


def random7():
    """batch 7, n_seg_max 5, ragged n_seg; t_from inside every plan"""
    inp = pack(random_rows(7, 5, seed=11, n_seg=[5, 1, 3, 2, 5, 4, 1]), 5)
    inp["t_from"] = np.array([0.0, 0.3, 1.7, -1.0, 2.5, 0.9, 5.0])
    return inp


def long5():
    """batch 5, n_seg_max 30: 150 slots, more than two waves with a partial last one"""
    inp = pack(random_rows(5, 30, seed=12, n_seg=[30, 17, 30, 1, 23]), 30)
    inp["t_from"] = np.array([0.0, 4.0, 11.0, 0.2, -np.inf])
    return inp


INVALID_ROWS = {1: "n_seg = 0", 2: "n_seg > n_seg_max", 4: "T = 0", 5: "NaN T", 7: "NaN coefficient", 8: "NaN t_from"}


def invalid9():
    """batch 9, n_seg_max 5: the invalid rows of INVALID_ROWS between valid neighbours (rows 0, 3, 6)"""
    inp = pack(random_rows(9, 5, seed=13, n_seg=[3, 2, 2, 4, 3, 3, 5, 2, 2]), 5)
    inp["t_from"] = np.zeros(9)
    inp["n_seg"][1], inp["n_seg"][2] = 0, 6
    inp["T"][4, 1] = 0.0
    inp["T"][5, 2] = np.nan
    inp["bez"][7, 1, 9] = np.nan
    inp["poly"][7, 1, 9] = np.nan
    inp["t_from"][8] = np.nan
    return inp


def shared_inputs():
    return dict(random7=random7(), crafted=crafted(), long5=long5(), invalid9=invalid9())
