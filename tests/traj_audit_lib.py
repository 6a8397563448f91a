"""Restatement of direct_traj_audit_batch (include/direct_ddp.h, "continuous-time audit"), written from the contract alone.

Two sides.  The EXACT side (exact_audit) works on rationals (fractions.Fraction: every double is one) and finds the
critical points with mpmath.polyroots at 60 digits; it is what tests/golden/make_audit_golden.py stores, as hi + lo pairs of
doubles.  The TOLERANCE side is NumPy: the absolute companion F of every item (the item's expression at the end of its
interval with every input replaced by its magnitude and every subtraction by an addition); the contract's bound is
|peak - exact| <= 24 u F, u = 2^-53.  Nothing here looks at the library or at traj_audit_math.h."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
TOL_UNITS = 24.0
VEL, ACC, JERK, CORRIDOR, INVALID = 1, 2, 4, 8, 256
ROW_FIELDS = ("vpeak", "apeak", "jpeak", "vnorm", "anorm", "jnorm", "cpeak")


def starts(T, n):
    return np.concatenate([[0.0], np.cumsum(np.asarray(T[:n], np.float64))])


def row_valid(n, T, coef, n_planes=None, planes=None):
    nm = T.shape[0]
    if n < 1 or n > nm:
        return False
    Tn = np.asarray(T[:n], np.float64)
    if not np.all(np.isfinite(Tn) & (Tn > 0.0)):
        return False
    if not np.all(np.isfinite(np.asarray(coef[:n], np.float64))):
        return False
    if planes is not None:
        pm = planes.shape[1]
        for i in range(n):
            k = int(n_planes[i])
            if k < 1 or k > pm or not np.all(np.isfinite(np.asarray(planes[i, :k], np.float64))):
                return False
    return True


# ---- exact side ---------------------------------------------------------------------------------------------------------
def seg_poly(coef18, T, src):
    """the three axes' coefficients in s (s in [0, T]) as Fractions: [3][6]"""
    T = Fraction(float(T))
    if src == "poly":
        a = [[Fraction(float(coef18[m * 3 + d])) for m in range(6)] for d in range(3)]
        return a
    out = []
    for d in range(3):
        w = [Fraction(float(coef18[d * 6 + j])) for j in range(6)]
        D = [w[0]]
        for _ in range(5):
            w = [w[j + 1] - w[j] for j in range(len(w) - 1)]
            D.append(w[0])
        out.append([T * math.comb(5, m) * D[m] / T ** m for m in range(6)])   # p(T tau) = T sum_m C(5,m) D_m tau^m, tau = s / T
    return out


def deriv(p, k=1):
    for _ in range(k):
        p = [p[i] * i for i in range(1, len(p))] or [Fraction(0)]
    return p


def pmul(a, b):
    r = [Fraction(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] += x * y
    return r


def padd(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0) for i in range(n)]


def peval(p, x):
    r = Fraction(0)
    for c in reversed(p):
        r = r * x + c
    return r


def candidates(g, T):
    """0, T and the real roots of the Fraction polynomial g in (0, T), as Fractions of their 60-digit values.  A point that is not
    quite a root does no harm: every candidate lies in [0, T], so no value taken there exceeds the true maximum."""
    import mpmath as mp
    mp.mp.dps = 60
    T = Fraction(T)
    g = list(g)
    while g and g[-1] == 0:
        g.pop()
    pts = [Fraction(0), T]
    if len(g) >= 2:
        scale = max(abs(c) for c in g)
        co = [mp.mpf(c.numerator) / mp.mpf(c.denominator) / (mp.mpf(scale.numerator) / mp.mpf(scale.denominator)) for c in reversed(g)]
        # in x = s / T the roots are O(1) whatever T is
        n = len(co) - 1
        Tm = mp.mpf(T.numerator) / mp.mpf(T.denominator)
        co = [c * Tm ** (n - i) for i, c in enumerate(co)]
        roots = mp.polyroots(co, maxsteps=2000, extraprec=2000)
        for z in roots:
            if abs(mp.im(z)) < mp.mpf(10) ** -12 and -mp.mpf(10) ** -12 < mp.re(z) < 1 + mp.mpf(10) ** -12:
                x = min(max(mp.re(z), mp.mpf(0)), mp.mpf(1))
                m, e = mp.frexp(x)
                pts.append(Fraction(int(mp.ldexp(m, 200)), 1 << 200) * Fraction(2) ** int(e) * T)
    return sorted(set(min(max(p, Fraction(0)), T) for p in pts))


def max_of(f, T, absolute):
    """(max over [0, T] of f or |f|, earliest s attaining it) for a Fraction polynomial f"""
    best, at = None, None
    for x in candidates(deriv(f), T):
        v = peval(f, x)
        v = abs(v) if absolute else v
        if best is None or v > best:
            best, at = v, x
    return best, at


def split(fr):
    """a Fraction (or an exact square root given as ('sqrt', Fraction)) as hi + lo doubles"""
    if isinstance(fr, tuple):
        import mpmath as mp
        mp.mp.dps = 60
        v = mp.sqrt(mp.mpf(fr[1].numerator) / mp.mpf(fr[1].denominator))
        hi = float(v)
        return hi, float(v - mp.mpf(hi))
    hi = float(fr)
    return hi, float(fr - Fraction(hi))


def exact_row(n, T, coef, src, n_planes=None, planes=None):
    """One valid row -> dict of exact results: Fractions (norms as ('sqrt', Fraction))."""
    seg_peak = []
    peaks = [Fraction(-1)] * 3
    norms2 = [Fraction(0)] * 3
    cbest = csecond = None
    gap = [Fraction(0)] * 3
    prev = None
    S = starts(T, n)
    for i in range(n):
        P = seg_poly(coef[i], T[i], src)
        Ti = Fraction(float(T[i]))
        row = []
        for k in (1, 2, 3):
            f = [deriv(P[d], k) for d in range(3)]
            v = max(max_of(f[d], Ti, True)[0] for d in range(3))
            row.append(v)
            peaks[k - 1] = max(peaks[k - 1], v)
            n2 = [Fraction(0)]
            for d in range(3):
                n2 = padd(n2, pmul(f[d], f[d]))
            norms2[k - 1] = max(norms2[k - 1], max_of(n2, Ti, False)[0])
        c_here = Fraction(0)
        if planes is not None:
            c_here = None
            for k in range(int(n_planes[i])):
                a, b, c, d = (Fraction(float(x)) for x in planes[i, k])
                g = [a * P[0][m] + b * P[1][m] + c * P[2][m] for m in range(6)]
                g[0] += d
                v, s = max_of(g, Ti, False)
                key = (-v, Fraction(float(S[i])) + s, i, k)      # larger value, earlier time, earlier segment, smaller plane
                if cbest is None or key < cbest:
                    cbest, csecond = key, (None if cbest is None else -cbest[0])
                elif csecond is None or v > csecond:
                    csecond = v
                c_here = v if c_here is None else max(c_here, v)
        row.append(c_here)
        seg_peak.append(row)
        if prev is not None:
            for k in range(3):
                j = max(abs(peval(deriv(prev[0][d], k), prev[1]) - deriv(P[d], k)[0]) for d in range(3))
                gap[k] = max(gap[k], j)
        prev = (P, Ti)
    r = dict(vpeak=peaks[0], apeak=peaks[1], jpeak=peaks[2], vnorm=("sqrt", norms2[0]), anorm=("sqrt", norms2[1]),
             jnorm=("sqrt", norms2[2]), seg_peak=seg_peak, gap=gap)
    if cbest is not None:
        r["cpeak"] = -cbest[0]
        r["c_where"] = (cbest[2], cbest[3])
        r["c_margin"] = float("inf") if csecond is None else float(-cbest[0] - csecond)   # best minus second-best (segment, plane) item
    return r


def exact_audit(n_seg, T, coef, src, n_planes=None, planes=None):
    """Exact outputs of a batch as hi / lo double arrays: X and X_lo for the row fields, seg_peak, gap; status, c_where."""
    T = np.asarray(T, np.float64)
    B, nm = T.shape
    coef = np.asarray(coef, np.float64).reshape(B, nm, 18)
    o = {"status": np.zeros(B, np.int32), "c_where": np.zeros((B, 2), np.int32), "t_total": np.zeros(B)}
    for f in ROW_FIELDS:
        o[f], o[f + "_lo"] = np.zeros(B), np.zeros(B)
    o["seg_peak"], o["seg_peak_lo"] = np.zeros((B, nm, 4)), np.zeros((B, nm, 4))
    o["gap"], o["gap_lo"] = np.zeros((B, 3)), np.zeros((B, 3))
    o["c_margin"] = np.full(B, np.inf)
    for b in range(B):
        n = int(n_seg[b])
        pl = None if planes is None else planes[b]
        if not row_valid(n, T[b], coef[b], None if planes is None else n_planes[b], pl):
            o["status"][b] = -1
            continue
        o["t_total"][b] = starts(T[b], n)[n]
        r = exact_row(n, T[b], coef[b], src, None if planes is None else n_planes[b], pl)
        for f in ROW_FIELDS:
            if f in r:
                o[f][b], o[f + "_lo"][b] = split(r[f])
        if "c_where" in r:
            o["c_where"][b] = r["c_where"]
            o["c_margin"][b] = r["c_margin"]
        for i in range(n):
            for q in range(4):
                o["seg_peak"][b, i, q], o["seg_peak_lo"][b, i, q] = split(r["seg_peak"][i][q])
        for k in range(3):
            o["gap"][b, k], o["gap_lo"][b, k] = split(r["gap"][k])
    return o


def exact_value_at(n, T, coef, src, what, t, n_planes=None, planes=None, c_where=None):
    """The exact item value (Fraction) at time t on the plan's clock: what = 0, 1, 2 the largest |d^(what+1) p_d| over the axes,
    3 the plane c_where of its segment.  t == S_i is the end of segment i - 1 and the start of segment i: the larger counts."""
    S = starts(T, n)
    i = int(min(max(np.searchsorted(S[:n], t, side="right") - 1, 0), n - 1))
    places = [(i, Fraction(float(t)) - Fraction(float(S[i])))]
    if i > 0 and t == S[i]:
        places.append((i - 1, Fraction(float(T[i - 1]))))
    best = None
    for i, s in places:
        s = min(max(s, Fraction(0)), Fraction(float(T[i])))
        P = seg_poly(coef[i], T[i], src)
        if what < 3:
            v = max(abs(peval(deriv(P[d], what + 1), s)) for d in range(3))
        else:
            if c_where[0] != i:
                continue
            a, b, c, d = (Fraction(float(x)) for x in planes[i, c_where[1]])
            v = a * peval(P[0], s) + b * peval(P[1], s) + c * peval(P[2], s) + d
        best = v if best is None else max(best, v)
    return best


# ---- tolerance side -----------------------------------------------------------------------------------------------------
def falling(m, k):
    return math.factorial(m) / math.factorial(m - k)


def companions(T, coef18, src, planes=None):
    """F of one segment: dict k -> [3] per axis for the derivatives k = 0..3 at the end of the interval, 'start' -> the same for
    k = 0..2 at its start, and 'planes' -> [n_planes]"""
    T = float(T)
    c = np.abs(np.asarray(coef18, np.float64))
    F = {}
    if src == "poly":
        A = c.reshape(6, 3)                                                   # |a_m| per axis
        for k in range(4):
            F[k] = sum(falling(m, k) * A[m] * T ** (m - k) for m in range(k, 6))
        F["start"] = [falling(k, k) * A[k] for k in range(3)]                 # the same expressions at s = 0
    else:
        w = c.reshape(3, 6)
        D = np.stack([sum(math.comb(m, i) * w[:, i] for i in range(m + 1)) for m in range(6)])   # [6][3]: sum_i C(m,i) |c_i|
        A = np.stack([math.comb(5, m) * D[m] for m in range(6)])
        for k in range(4):
            F[k] = T ** (1 - k) * sum(falling(m, k) * A[m] for m in range(k, 6))
        F["start"] = [T ** (1 - k) * falling(k, k) * A[k] for k in range(3)]
    if planes is not None:
        p = np.abs(np.asarray(planes, np.float64))
        F["planes"] = p[:, :3] @ F[0] + p[:, 3]
    return F


def tolerances(n_seg, T, coef, src, n_planes=None, planes=None):
    """24 u F per output: dict of the row fields [B], seg_peak [B][nm][4] (the largest F among the items an entry is the maximum of)"""
    T = np.asarray(T, np.float64)
    B, nm = T.shape
    coef = np.asarray(coef, np.float64).reshape(B, nm, 18)
    o = {f: np.zeros(B) for f in ROW_FIELDS}
    o["seg_peak"] = np.zeros((B, nm, 4))
    o["gap"] = np.zeros((B, 3))
    for b in range(B):
        n = int(n_seg[b])
        if n < 1 or n > nm:
            continue
        Fprev = None
        for i in range(n):
            pl = None if planes is None else planes[b, i, :max(int(n_planes[b, i]), 0)]
            with np.errstate(invalid="ignore", over="ignore"):     # invalid rows may hold anything
                F = companions(T[b, i], coef[b, i], src, pl)
            for q, k in enumerate((1, 2, 3)):
                o["seg_peak"][b, i, q] = F[k].max()
                o[ROW_FIELDS[3 + q]][b] = max(o[ROW_FIELDS[3 + q]][b], np.linalg.norm(F[k]))
            if pl is not None and len(pl):
                o["seg_peak"][b, i, 3] = F["planes"].max()
            if Fprev is not None:
                for k in range(3):
                    o["gap"][b, k] = max(o["gap"][b, k], (Fprev[k] + F["start"][k]).max())   # end of i - 1 against the start of i
            Fprev = F
        for q in range(3):
            o[ROW_FIELDS[q]][b] = o["seg_peak"][b, :n, q].max()
        o["cpeak"][b] = o["seg_peak"][b, :n, 3].max()
    return {k: TOL_UNITS * U * v for k, v in o.items()}


def verdict(peaks, limits, has_planes):
    """item 6: peaks = (v, a, j, c) judged, limits = (max_vel, max_acc, max_jerk, clearance)"""
    w = 0
    for bit, p, l in zip((VEL, ACC, JERK), peaks[:3], limits[:3]):
        if l > 0 and p > l:
            w |= bit
    if has_planes and peaks[3] > -limits[3]:
        w |= CORRIDOR
    return w


def slowdown(peaks, limits):
    s = 1.0
    for p, l, e in zip(peaks[:3], limits[:3], (1.0, 0.5, 1.0 / 3.0)):
        if l > 0:
            s = max(s, (p / l) ** e)
    return s


def best_row(cost, verdicts, rtn=None):
    ok = np.asarray(verdicts) == 0
    if rtn is not None:
        ok &= np.asarray(rtn) >= 0
    if not ok.any():
        return -1
    c = np.where(ok, np.asarray(cost, np.float64), np.inf)
    return int(np.argmin(c))


def poly_in_s(coef18, T, src):
    """[6][3] float coefficients in s of one segment (NumPy, for dense sampling and control polygons)"""
    return np.array([[float(x) for x in ax] for ax in seg_poly(coef18, T, src)]).T


def dense_values(a, T, k, m=2000):
    """[m][3] values of the k-th derivative of the [6][3] polynomial a at m points of [0, T], both ends included"""
    s = np.linspace(0.0, float(T), m)
    out = np.zeros((m, 3))
    for q in range(5, k - 1, -1):
        out = out * s[:, None] + falling(q, k) * a[q]
    return out


def control_polygon(a, T, k):
    """[6-k][3] Bernstein coefficients on [0, T] of the k-th derivative of the [6][3] polynomial a"""
    N = 5 - k
    f = np.array([falling(q + k, k) * a[q + k] * float(T) ** q for q in range(N + 1)])
    return np.array([sum(math.comb(j, q) / math.comb(N, q) * f[q] for q in range(j + 1)) for j in range(N + 1)])


def sandwich(n_seg, T, coef, src, seg_peak, tol, n_planes=None, planes=None, rows=None):
    """The bracket that needs no oracle, per segment: the largest of 2000 dense samples <= the audited peak + tol, and the audited
    peak <= the largest magnitude over the control polygon of that derivative (convex-hull property) + tol; for the planes, the
    same against the position's control points.  seg_peak, tol: [B][nm][4]."""
    for b in (range(len(n_seg)) if rows is None else rows):
        for i in range(int(n_seg[b])):
            a = poly_in_s(coef[b, i], T[b, i], src)
            for q, k in enumerate((1, 2, 3)):
                got, t = seg_peak[b, i, q], tol[b, i, q]
                assert np.abs(dense_values(a, T[b, i], k)).max() <= got + t, (b, i, k)
                assert got <= np.abs(control_polygon(a, T[b, i], k)).max() + t, (b, i, k)
            if planes is not None:
                pl = np.asarray(planes[b, i, :int(n_planes[b, i])], np.float64)
                got, t = seg_peak[b, i, 3], tol[b, i, 3]
                assert (dense_values(a, T[b, i], 0) @ pl[:, :3].T + pl[:, 3]).max() <= got + t, (b, i)
                assert got <= (control_polygon(a, T[b, i], 0) @ pl[:, :3].T + pl[:, 3]).max() + t, (b, i)


def fixture_case(fix, name, golden_dir):
    """One case of tests/golden/audit_cases.npz as a dict: the exact outputs it stores and its inputs.  Synthetic cases store
    their inputs; a case made from a solved plan, "<golden>_<p0|p1>_<f64|f32>_<poly|bez>", takes them from tests/golden/<golden>.npz
    (f32: rounded to float, held in double arrays)."""
    import os
    pre = name + "/"
    c = {k[len(pre):]: fix[k] for k in fix.files if k.startswith(pre)}
    c["src"] = name.rsplit("_", 1)[1]
    if "n_seg" not in c:
        plan, ph, prec, src = name.rsplit("_", 3)
        g = np.load(os.path.join(golden_dir, plan + ".npz"))
        r = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if prec == "f32" else (lambda a: np.asarray(a, np.float64))
        c.update(n_seg=g["n_seg"].astype(np.int32), T=r(g[ph + "_T"]), coef=r(g[ph + "_" + src]),
                 n_planes=g["n_planes"].astype(np.int32), planes=r(g["planes"]))
    c.setdefault("n_planes", None)
    c.setdefault("planes", None)
    return c
