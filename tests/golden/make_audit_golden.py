"""Writes tests/golden/audit_cases.npz: inputs and EXACT outputs (tests/traj_audit_lib.py, rationals + mpmath.polyroots at
60 digits) of direct_traj_audit_batch, so that the suite does not pay for mpmath on every run.

    python tests/golden/make_audit_golden.py          (about ten CPU-minutes, spread over the machine's cores)

Keys are "<case>/<field>".  Inputs of the synthetic cases: n_seg, T, coef ([B][nm][18], of the source the case's name ends in),
and n_planes, planes where the case has a corridor.  The cases made from solved plans store no inputs: they are the committed
goldens tests/golden/<plan>.npz, in double or rounded to float (tests/traj_audit_lib.py, fixture_case).  Outputs: status, t_total, c_where, and hi / lo
pairs X, X_lo (exact = X + X_lo) of the seven row peaks, seg_peak and gap.  `cases` lists the names; `plan_cases` those made
from solved plans (the verdict check of tests/test_traj_audit_restatement.py uses only them)."""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import traj_audit_lib as L  # noqa: E402

PLANS = ("corridor_n8", "corridor_n20", "free_n5", "config1_n50", "free_n6_tp1")


def to_bez(poly, T):
    """time-scaled control points [18] of the segment with getPolyCoeff() rows poly [6][3]: c_j = sum_m C(j,m)/C(5,m) a_m T^m / T"""
    M = np.array([[math.comb(j, m) / math.comb(5, m) if j >= m else 0.0 for m in range(6)] for j in range(6)])
    return ((M @ (poly * (T ** np.arange(6))[:, None])).T / T).reshape(18)


def synthetic():
    """rows of up to 3 segments as (n, T[3], poly[3][6][3])"""
    rng = np.random.default_rng(11)
    rows = []

    def seg(x=(), y=(), z=()):
        a = np.zeros((6, 3))
        for d, c in enumerate((x, y, z)):
            a[:len(c), d] = c
        return a

    def row(T, *segs):
        n = len(segs)
        P = np.zeros((3, 6, 3))
        P[:n] = segs
        TT = np.ones(3)
        TT[:n] = T
        rows.append((n, TT, P))

    row([1.5], seg([2.0], [-3.0], [0.5]))                                     # a constant, n = 1
    row([1.0, 2.0], seg([0, 1.0], [1, -2.0], [0, 0.5]), seg([1, 1.0], [-1, -2.0], [0.5, 0.5]))   # a line
    row([2.0], seg([0, 0, 0, 0, 0, 1.0], [0, 0, 2.0], [3.0, -1.0]))           # s^5, 2 s^2, 3 - s
    # v(s) = 1 - 4 (s - 0.25)^2: the peak lies strictly between the dt = 0.1 samples 0.2 and 0.3
    # (|v| stays below 1 up to the end of the segment at 0.6); y = s / 2 - s^2 peaks there too, with 0.0625
    row([0.6], seg([0, 0.75, 1.0, -4.0 / 3.0], [0, 0.5, -1.0]))
    row([0.75, 0.5], seg([0, 0.1, 0.5, 0.3, 0.2]), seg([0, 1.0, 0, -0.2]))      # monotone velocity: the peak at a segment end
    for delta in (1e-9, 1e-7, 1e-5, 1e-3):                                    # two critical points of the velocity delta T apart
        T, s0 = 2.0, 0.7
        d = delta * T
        # acc = (s - s0)(s - s0 - d) -> vel = its integral + 0.3
        a2, a1, a0 = 1.0, -(2 * s0 + d), s0 * (s0 + d)
        row([T], seg([0, 0.3, a0 / 2, a1 / 6, a2 / 12], [0, 0, 0, 0, a0 / 12, a1 / 20 + 0.01]))
    for T in (0.01, 0.3, 10.0, 100.0):
        c = rng.standard_normal((3, 6, 3)) / (T ** np.arange(6))[None, :, None]
        row([T, T * 1.5, T * 0.5], *c)
    for k in range(3):                                                        # coefficients spread over 12 decades
        c = rng.standard_normal((2, 6, 3)) * 10.0 ** rng.uniform(-6, 6, (2, 6, 3))
        row([1.0, 0.9], *c)
    n = np.array([r[0] for r in rows], np.int32)
    return n, np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])


def synthetic_planes(n, T, P):
    """corridors for the synthetic rows: neutral planes everywhere, then a touched and a crossed plane on two rows"""
    B = len(n)
    planes = np.zeros((B, 3, 4, 4))
    planes[..., 3] = -1.0
    npl = np.full((B, 3), 3, np.int32)
    # row 3: y = s / 2 - s^2 peaks at s = 1/4 with 0.0625: the plane y - 0.0625 <= 0 is touched there
    planes[3, 0, 1] = (0.0, 1.0, 0.0, -0.0625)
    # row 1 (a line, two segments): x = s then 1 + s: the plane x - 1.5 <= 0 is crossed in the second segment only
    planes[1, 0, 2] = (1.0, 0.0, 0.0, -1.5)
    planes[1, 1, 0] = (1.0, 0.0, 0.0, -1.5)
    return npl, planes


def invalid_rows(n, T, P):
    """every invalid-row kind around valid copies of synthetic row 4 -> n_seg, T, poly, n_planes, planes (row 0 and the last stay valid)"""
    B = 13
    nn, TT, PP = np.repeat(n[4:5], B), np.repeat(T[4:5], B, 0), np.repeat(P[4:5], B, 0)
    planes = np.zeros((B, 3, 4, 4))
    planes[..., 3] = -1.0
    npl = np.full((B, 3), 2, np.int32)
    nn[1], nn[2] = 0, 4
    TT[3, 1], TT[4, 0], TT[5, 1], TT[6, 0] = 0.0, -0.5, np.inf, np.nan
    PP[7, 1, 3, 2], PP[8, 0, 0, 0] = np.nan, np.inf
    npl[9, 1], npl[10, 0] = 0, 5
    planes[9, 2, 1, 0] = np.nan          # past n_seg: never read (row 9 is invalid through its n_planes alone)
    planes[0, 0, 3, 1] = np.nan          # past n_planes: never read, row 0 stays valid
    PP[0, 2] = np.nan                    # past n_seg: never read
    planes[10, 1, 1, 2] = np.inf
    planes[11, 1, 1, 3] = np.inf         # every n_planes entry valid: invalid ONLY through plane 1 < n_planes of segment 1 < n_seg
    planes[12, 1, 1, 3] = -2.0           # finite: the last row stays valid
    return nn, TT, PP, npl, planes


def one_row(args):
    n, T, coef, src, npl, planes = args
    return L.exact_audit(n, T, coef, src, npl, planes)


def main():
    cases = {}
    plan_cases = []
    for name in PLANS:
        g = np.load(os.path.join(HERE, name + ".npz"))
        for ph in ("p0", "p1"):
            for src in ("poly", "bez"):
                for prec, dt in (("f64", np.float64), ("f32", np.float32)):
                    key = "%s_%s_%s_%s" % (name, ph, prec, src)
                    r = lambda a: np.asarray(a, dt).astype(np.float64)
                    cases[key] = dict(n_seg=g["n_seg"].astype(np.int32), T=r(g[ph + "_T"]), coef=r(g[ph + "_" + src]),
                                      n_planes=g["n_planes"].astype(np.int32), planes=r(g["planes"]))
                    plan_cases.append(key)
    n, T, P = synthetic()
    npl, planes = synthetic_planes(n, T, P)
    B = len(n)
    bez = np.stack([[to_bez(P[b, i], T[b, i]) for i in range(3)] for b in range(B)])
    cases["synthetic_poly"] = dict(n_seg=n, T=T, coef=P.reshape(B, 3, 18), n_planes=npl, planes=planes)
    cases["synthetic_bez"] = dict(n_seg=n, T=T, coef=bez, n_planes=npl, planes=planes)
    cases["synthetic_free_poly"] = dict(n_seg=n, T=T, coef=P.reshape(B, 3, 18))
    ni, Ti, Pi, npi, pli = invalid_rows(n, T, P)
    cases["invalid_poly"] = dict(n_seg=ni, T=Ti, coef=Pi.reshape(len(ni), 3, 18), n_planes=npi, planes=pli)
    tasks, where = [], []
    for key, c in cases.items():
        for b in range(len(c["n_seg"])):
            pl = "planes" in c
            tasks.append((c["n_seg"][b:b + 1], c["T"][b:b + 1], c["coef"][b:b + 1], key.rsplit("_", 1)[1],
                          c["n_planes"][b:b + 1] if pl else None, c["planes"][b:b + 1] if pl else None))
            where.append(key)
    with Pool(min(32, os.cpu_count() or 1)) as pool:
        res = pool.map(one_row, tasks, chunksize=1)
    out = {"cases": np.array(list(cases)), "plan_cases": np.array(plan_cases)}
    for key, c in cases.items():
        rows = [r for r, w in zip(res, where) if w == key]
        ex = {f: np.concatenate([r[f] for r in rows]) for f in rows[0]}
        margin = ex.pop("c_margin")
        if "planes" in c:   # no near-ties between planes: an exact tie (neutral planes) or a clear gap
            ok = (ex["status"] != 0) | (margin == 0.0) | (margin >= 1e-6)
            assert ok.all(), (key, margin)
        else:
            for f in ("cpeak", "cpeak_lo", "c_where"):
                ex.pop(f)
        stored = {} if key in plan_cases else c      # a plan's inputs are tests/golden/<plan>.npz: traj_audit_lib.fixture_case
        for f, v in list(stored.items()) + list(ex.items()):
            out[key + "/" + f] = v
    np.savez_compressed(os.path.join(HERE, "audit_cases.npz"), **out)
    print("wrote %d cases, %d rows" % (len(cases), len(tasks)))


if __name__ == "__main__":
    main()
