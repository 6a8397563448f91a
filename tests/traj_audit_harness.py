"""g++ build of direct_amd/csrc/traj_audit_math.h as a program: the sequence of calls the kernels of traj_audit.h make, one row
after the other on the CPU.  tests/test_traj_audit_restatement.py checks it against the exact fixture; the GPU tests ask the
kernels for the same bits."""
import os
import subprocess

import numpy as np

from tests.cpp_program import compile_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r'''
#include <cstdio>
#include <vector>
#include "traj_audit_math.h"
using namespace direct::audit;
// in: int32 B, nmax, pmax (0: no corridor), poly, norms, on_norm, has_cost, has_rtn; float64 max_vel, max_acc, max_jerk, clearance;
//     int32 n_seg[B]; float64 T[B][nmax], coef[B][nmax][18]; int32 n_planes[B][nmax]; float64 planes[B][nmax][pmax][4], cost[B]; int32 rtn[B]
// out: per row 22 float64 (status, t_total, 7 peaks, c_where[2], at[4], gap[3], verdict, slowdown, pad) and seg_peak[nmax][4]; then best
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  int h[8]; double g[4];
  if (!f || fread(h, 4, 8, f) != 8 || fread(g, 8, 4, f) != 4) return 1;
  const int B = h[0], nm = h[1], pm = h[2], poly = h[3], norms = h[4];
  const Limits lim{g[0], g[1], g[2], g[3], h[5], pm > 0};
  std::vector<int> n_seg(B), n_planes((size_t)B * nm), rtn(B);
  std::vector<double> T((size_t)B * nm), coef((size_t)B * nm * 18), planes((size_t)B * nm * pm * 4), cost(B);
  if (fread(n_seg.data(), 4, B, f) != (size_t)B || fread(T.data(), 8, T.size(), f) != T.size() ||
      fread(coef.data(), 8, coef.size(), f) != coef.size() || fread(n_planes.data(), 4, n_planes.size(), f) != n_planes.size() ||
      fread(planes.data(), 8, planes.size(), f) != planes.size() || fread(cost.data(), 8, B, f) != (size_t)B ||
      fread(rtn.data(), 4, B, f) != (size_t)B) return 1;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  std::vector<double> S(nm + 1), sp((size_t)nm * 4);
  double best_cost = 0.0, best = -1.0;
  for (int b = 0; b < B; b++) {
    const int n = n_seg[b];
    int ok = direct::eval::row_starts(&T[(size_t)b * nm], n, nm, S.data());
    double head[22] = {0.0};
    std::fill(sp.begin(), sp.end(), 0.0);
    RowAcc A;
    row_init(A);
    double prev[kRec], rec[kRec];
    for (int i = 0; ok && i < n; i++) {
      const size_t gi = (size_t)b * nm + i;
      const double* c = &coef[gi * 18];
      int bad = 0;
      for (int q = 0; q < 18; q++) bad |= !is_finite(c[q]);
      if (poly) seg_from_poly(c, T[gi], S[i], rec); else seg_from_bez(c, T[gi], S[i], rec);
      double w[kWs];
      segment_items(rec, i ? prev : nullptr, norms, w);
      if (pm) {
        const int np = n_planes[gi];
        if (np < 1 || np > pm) bad = 1;
        for (int k = 0; !bad && k < np; k++) {
          const double* p = &planes[(gi * pm + k) * 4];
          if (!(is_finite(p[0]) && is_finite(p[1]) && is_finite(p[2]) && is_finite(p[3]))) { bad = 1; break; }
          double v, t;
          plane_peak(rec, p[0], p[1], p[2], p[3], v, t);
          segment_plane(w, k, v, t);
        }
      }
      w[W_BAD] = bad;
      row_add(A, i, w, pm > 0);
      for (int q = 0; q < 4; q++) sp[(size_t)i * 4 + q] = w[q];
      for (int q = 0; q < kRec; q++) prev[q] = rec[q];
    }
    ok = ok && !A.bad;
    if (!ok) {
      std::fill(sp.begin(), sp.end(), 0.0);
      head[0] = -1.0;
      head[20] = DIRECT_AUDIT_INVALID;
    } else {
      RowOut R;
      row_finish(A, lim, R);
      head[1] = S[n];
      for (int q = 0; q < 7; q++) head[2 + q] = R.peak[q];
      head[9] = R.c_where[0]; head[10] = R.c_where[1];
      for (int q = 0; q < 4; q++) head[11 + q] = R.at[q];
      for (int q = 0; q < 3; q++) head[15 + q] = R.gap[q];
      head[18] = R.verdict; head[19] = R.slowdown; head[20] = R.verdict;
      if (h[6] && R.verdict == 0 && (!h[7] || rtn[b] >= 0) && cost[b] == cost[b] && (best < 0.0 || cost[b] < best_cost)) { best = b; best_cost = cost[b]; }
    }
    fwrite(head, 8, 22, o);
    fwrite(sp.data(), 8, sp.size(), o);
  }
  fwrite(&best, 8, 1, o);
  fclose(o);
  return 0;
}
'''

ROW_FIELDS = ("vpeak", "apeak", "jpeak", "vnorm", "anorm", "jnorm", "cpeak")


def build(workdir):
    return str(workdir), compile_program(workdir, "audit_harness", HARNESS)


def run(harness, n_seg, T, coef, src, n_planes=None, planes=None, limits=(0.0, 0.0, 0.0, 0.0), on_norm=0, norms=1, cost=None,
        rtn=None):
    """-> dict of float64 / int arrays with the library's output names (all computed; `best` = -1 without cost)"""
    d, exe = harness
    T = np.ascontiguousarray(T, np.float64)
    B, nm = T.shape
    pm = 0 if planes is None else planes.shape[2]
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        np.array([B, nm, pm, int(src == "poly"), int(norms), int(on_norm), int(cost is not None), int(rtn is not None)], np.int32).tofile(f)
        np.array(limits, np.float64).tofile(f)
        np.asarray(n_seg, np.int32).tofile(f)
        T.tofile(f)
        np.ascontiguousarray(coef, np.float64).reshape(B, nm, 18).tofile(f)
        (np.zeros((B, nm), np.int32) if planes is None else np.ascontiguousarray(n_planes, np.int32)).tofile(f)
        if planes is not None:
            np.ascontiguousarray(planes, np.float64).tofile(f)
        (np.zeros(B) if cost is None else np.ascontiguousarray(cost, np.float64)).tofile(f)
        (np.zeros(B, np.int32) if rtn is None else np.ascontiguousarray(rtn, np.int32)).tofile(f)
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, np.float64)
    rows = raw[:-1].reshape(B, 22 + nm * 4)
    r = dict(status=rows[:, 0].astype(np.int32), t_total=rows[:, 1].copy(), c_where=rows[:, 9:11].astype(np.int32),
             at=rows[:, 11:15].copy(), gap=rows[:, 15:18].copy(), verdict=rows[:, 20].astype(np.int32), slowdown=rows[:, 19].copy(),
             seg_peak=rows[:, 22:].reshape(B, nm, 4).copy(), best=np.array([int(raw[-1])], np.int64))
    for q, name in enumerate(ROW_FIELDS):
        r[name] = rows[:, 2 + q].copy()
    return r
