"""NumPy restatement of direct_traj_eval_batch (include/direct_ddp.h, "trajectory evaluation"), written from the contract
alone: segment start times by numpy.cumsum, the segment by searchsorted, Bernstein sums over the k-th differences of the
control points (bez) and the derivatives of the monomial (poly).  Double arithmetic; results are the host-memory ones
(entries past n_query read zero)."""
import math

import numpy as np

NAMES = ("pos", "vel", "acc", "jerk", "snap")
FACT = (1.0, 5.0, 20.0, 60.0, 120.0)   # 5! / (5 - k)!
GAUSS3 = (np.array([-math.sqrt(0.6), 0.0, math.sqrt(0.6)]), np.array([5.0, 8.0, 5.0]) / 9.0)


def starts(T, n):
    """S[0..n]: 0, T_0, T_0 + T_1, ... summed left to right in double"""
    return np.concatenate([[0.0], np.cumsum(np.asarray(T[:n], np.float64))])


def row_valid(n, T, n_seg_max):
    if n < 1 or n > n_seg_max:
        return False
    Tn = np.asarray(T[:n], np.float64)
    return bool(np.all(np.isfinite(Tn) & (Tn > 0.0)))


def grid_times(m, t0, dt):
    return t0 + np.arange(m) * dt


def locate(S, n, t):
    """(seg, t_c) of every time: seg = largest i in [0, n-1] with S_i <= t_c; NaN -> seg -1"""
    t = np.asarray(t, np.float64)
    nan = np.isnan(t)
    tc = np.minimum(np.maximum(np.where(nan, 0.0, t), 0.0), S[n])
    seg = np.searchsorted(S[:n], tc, side="right") - 1
    return np.where(nan, -1, seg), np.where(nan, np.nan, tc)


def bez_derivs(c, T, tau):
    """c [q][3][6] time-scaled control points, T [q], tau [q] -> [5][q][3]: T^(1-k) 5!/(5-k)! sum_j Delta^k c_j B_j^(5-k)(tau)"""
    c, T, tau = np.asarray(c, np.float64), np.asarray(T, np.float64), np.asarray(tau, np.float64)
    out = np.zeros((5,) + c.shape[:2])
    for k in range(5):
        deg = 5 - k
        dk = np.diff(c, n=k, axis=-1)
        j = np.arange(deg + 1)
        basis = np.array([math.comb(deg, i) for i in j]) * tau[:, None] ** j * (1.0 - tau[:, None]) ** (deg - j)
        out[k] = T[:, None] ** (1 - k) * FACT[k] * np.einsum("qdj,qj->qd", dk, basis)
    return out


def poly_derivs(a, s):
    """a [q][6][3] (row m = coefficient of s^m), s [q] -> [5][q][3]"""
    a, s = np.asarray(a, np.float64), np.asarray(s, np.float64)
    out = np.zeros((5, a.shape[0], 3))
    for k in range(5):
        acc = np.zeros((a.shape[0], 3))
        for m in range(5, k - 1, -1):
            acc = acc * s[:, None] + (math.factorial(m) / math.factorial(m - k)) * a[:, m, :]
        out[k] = acc
    return out


def evaluate(n_seg, T, bez=None, poly=None, times=None, t0=0.0, dt=None, m=None, n_query=None):
    """The contract for a batch: dict of status, t_total, seg, pos .. snap [B][m][3], state [B][m][9]."""
    assert (bez is None) != (poly is None)
    T = np.asarray(T, np.float64)
    B, nm = T.shape
    if times is not None:
        times = np.asarray(times, np.float64).reshape(B, -1)
        m = times.shape[1]
    r = dict(status=np.zeros(B, np.int32), t_total=np.zeros(B), seg=np.zeros((B, m), np.int32), state=np.zeros((B, m, 9)))
    for k in NAMES:
        r[k] = np.zeros((B, m, 3))
    for b in range(B):
        nq = m if n_query is None else min(max(int(n_query[b]), 0), m)
        n = int(n_seg[b])
        if not row_valid(n, T[b], nm):
            r["status"][b] = -1
            r["seg"][b, :nq] = -1
            continue
        S = starts(T[b], n)
        r["t_total"][b] = S[n]
        t = times[b, :nq] if times is not None else grid_times(m, t0, dt)[:nq]
        seg, tc = locate(S, n, t)
        ok = seg >= 0
        i = np.where(ok, seg, 0)
        if bez is not None:
            c = np.asarray(bez, np.float64)[b, i].reshape(-1, 3, 6)
            d = bez_derivs(c, T[b, i], np.minimum((tc - S[i]) / T[b, i], 1.0))
        else:
            d = poly_derivs(np.asarray(poly, np.float64)[b, i].reshape(-1, 6, 3), tc - S[i])
        d[:, ~ok] = np.nan
        r["seg"][b, :nq] = seg
        for k, name in enumerate(NAMES):
            r[name][b, :nq] = d[k]
        r["state"][b, :nq] = np.concatenate([d[0], d[1], d[2]], axis=1)
    return r


def gauss_times(n_seg, T):
    """[B][3 n_seg_max] the 3-point Gauss-Legendre nodes of every segment on the trajectory's clock (NaN past n_seg), and
    the matching weights times T_i / 2"""
    T = np.asarray(T, np.float64)
    B, nm = T.shape
    x, w = GAUSS3
    t = np.full((B, nm, 3), np.nan)
    wt = np.zeros((B, nm, 3))
    for b in range(B):
        n = int(n_seg[b])
        S = starts(T[b], n)
        t[b, :n] = S[:n, None] + 0.5 * T[b, :n, None] * (1.0 + x)
        wt[b, :n] = 0.5 * T[b, :n, None] * w
    return t.reshape(B, -1), wt.reshape(B, -1)


def jerk_cost(jerk, wt):
    """sum over segments of the integral of |jerk|^2 (exact for the degree-4 integrand) from jerk at gauss_times"""
    j2 = np.nan_to_num((np.asarray(jerk, np.float64) ** 2).sum(-1))
    return (j2 * wt).sum(1)


def sampler_times(n_seg, T, dt, capacity):
    """Absolute times S_i + tau T_i of the stored samples of the sampler's loop (tau from the reference's accumulation
    t += dt / T_i) -> [B][capacity] (NaN where nothing is stored)"""
    T = np.asarray(T, np.float64)
    B = T.shape[0]
    out = np.full((B, capacity), np.nan)
    for b in range(B):
        n = int(n_seg[b])
        S = starts(T[b], n)
        q = 0
        for i in range(n):
            tau, step = 0.0, dt / float(T[b, i])
            while tau < 1.0:
                if q < capacity:
                    out[b, q] = S[i] + tau * T[b, i]
                q += 1
                tau += step
    return out
