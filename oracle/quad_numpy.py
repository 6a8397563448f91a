"""TEST INFRASTRUCTURE: an independent NumPy restatement of the BASELINE-label model (include/direct_quad.h), as pure
per-pass functions.  Written from the model in the header, not from oracle/quad_ref.c or the kernel:

  * the thrust direction is e3 turned by Rx(phi), Ry(theta), Rz(psi) one after the other, the Euler rates come from
    inverting omega = E(phi, theta) eulerdot, omegadot from an explicit cross product;
  * the Jacobians are obtained by COMPLEX-STEP differentiation of `dynamics` (no hand-expanded derivative anywhere);
  * the backward sweep is the dense textbook recursion with np.matmul.

Every function takes arrays with a leading batch axis and an arithmetic `dtype` (np.float64 or np.longdouble); `store`
(np.float64 or np.float32) is the storage type of the iterate and the gains: values are rounded to it exactly where
the device rounds them (u before use, x_{k+1} before it is used and stored, the initial roll likewise, gains when
they are written; the value recursion keeps the unrounded gains).  The hover input uh of the cost is the double
product m * g; the initial roll applies it rounded to `store`, like every later input.
"""
import numpy as np

LD = np.longdouble
NX, NU = 12, 4
N_STEPS = 11
REG_MAX = 24
MAX_RETRIES = 30


def _real(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.clongdouble:
        return np.dtype(LD)
    if dtype == np.complex128:
        return np.dtype(np.float64)
    return dtype


def _cplx(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(LD) else np.complex128


def rs(a, store, dtype):
    """round to the storage type, back in the arithmetic type"""
    return np.asarray(a, dtype).astype(store).astype(dtype)


class Consts:
    def __init__(self, p, dtype):
        t = _real(dtype).type
        self.m, self.g, self.dt = t(p.mass), t(p.gravity), t(p.dt)
        self.J = np.array([p.inertia[0], p.inertia[1], p.inertia[2]], t)
        self.q = np.repeat(np.array([p.q_pos, p.q_vel, p.q_ang, p.q_rate], t), 3)
        self.qf = np.repeat(np.array([p.qf_pos, p.qf_vel, p.qf_ang, p.qf_rate], t), 3)
        self.r = np.array([p.r_thrust, p.r_torque, p.r_torque, p.r_torque], t)
        self.uh = np.array([np.float64(p.mass) * np.float64(p.gravity), 0, 0, 0], t)
        self.reg_base = t(p.reg_base)


def dynamics(p, x, u, dtype=np.float64, with_abs=False):
    """f(x, u) for x[..., 12], u[..., 4] in `dtype` (float64, longdouble or their complex kinds).  with_abs: also the
    sum of the absolute values of the terms of every component (the scale of its rounding error)."""
    c = Consts(p, dtype)
    x, u = np.asarray(x, dtype), np.asarray(u, dtype)
    lead = np.broadcast_shapes(x.shape[:-1], u.shape[:-1])
    x, u = np.broadcast_to(x, lead + (NX,)), np.broadcast_to(u, lead + (NU,))
    v, w = x[..., 3:6], x[..., 9:12]
    sph, cph, sth, cth, sps, cps = (np.sin(x[..., 6]), np.cos(x[..., 6]), np.sin(x[..., 7]), np.cos(x[..., 7]),
                                    np.sin(x[..., 8]), np.cos(x[..., 8]))
    # R e3: e3 turned about x by phi, then about y by theta, then about z by psi
    bx, by, bz = 0 * sph, -sph, cph
    bx, bz = bx * cth + bz * sth, -bx * sth + bz * cth
    t1, t2, t3, t4 = bx * cps, -by * sps, bx * sps, by * cps
    a = u[..., 0] / c.m
    acc = [a * (t1 + t2), a * (t3 + t4), a * bz - c.g]
    # omega = E eulerdot, E = [[1, 0, -s_th], [0, c_ph, s_ph c_th], [0, -s_ph, c_ph c_th]]
    e1, e2 = sph * w[..., 1], cph * w[..., 2]
    psd = (e1 + e2) / cth
    thd = cph * w[..., 1] - sph * w[..., 2]
    phd = w[..., 0] + sth * psd
    # J omegadot = tau - omega x (J omega)
    Jw = c.J * w
    cr = [w[..., 1] * Jw[..., 2] - w[..., 2] * Jw[..., 1], w[..., 2] * Jw[..., 0] - w[..., 0] * Jw[..., 2],
          w[..., 0] * Jw[..., 1] - w[..., 1] * Jw[..., 0]]
    wd = [(u[..., 1 + i] - cr[i]) / c.J[i] for i in range(3)]
    f = np.stack([v[..., 0], v[..., 1], v[..., 2], acc[0], acc[1], acc[2], phd, thd, psd, wd[0], wd[1], wd[2]], axis=-1)
    if not with_abs:
        return f
    ab = np.abs
    ca = [ab(w[..., 1] * Jw[..., 2]) + ab(w[..., 2] * Jw[..., 1]), ab(w[..., 2] * Jw[..., 0]) + ab(w[..., 0] * Jw[..., 2]),
          ab(w[..., 0] * Jw[..., 1]) + ab(w[..., 1] * Jw[..., 0])]                  # both products of the cross product
    fa = np.stack([ab(v[..., 0]), ab(v[..., 1]), ab(v[..., 2]),
                   ab(a) * (ab(t1) + ab(t2)), ab(a) * (ab(t3) + ab(t4)), ab(a * bz) + c.g,
                   ab(w[..., 0]) + ab(sth / cth) * (ab(e1) + ab(e2)), ab(cph * w[..., 1]) + ab(sph * w[..., 2]),
                   (ab(e1) + ab(e2)) / ab(cth)] +
                  [(ab(u[..., 1 + i]) + ca[i]) / c.J[i] for i in range(3)], axis=-1)
    return f, fa


def step(p, x, u, dtype=np.float64):
    return np.asarray(x, dtype) + Consts(p, dtype).dt * dynamics(p, x, u, dtype)


def jacobians(p, x, u, dtype=np.float64):
    """Dense A = I + dt f_x [..., 12, 12] and B = dt f_u [..., 12, 4] by complex-step differentiation of `dynamics`
    (f is analytic; with h = 1e-40 the result is exact to the rounding of one evaluation)."""
    ct, rt = _cplx(dtype), _real(dtype).type
    h = rt(1e-40)
    x, u = np.asarray(x, dtype), np.asarray(u, dtype)
    xc = x[..., None, :].astype(ct) + 1j * h * np.eye(NX, dtype=dtype)
    fx = dynamics(p, xc, u[..., None, :].astype(ct), ct).imag / h          # [..., j, i]
    uc = u[..., None, :].astype(ct) + 1j * h * np.eye(NU, dtype=dtype)
    fu = dynamics(p, x[..., None, :].astype(ct), uc, ct).imag / h
    dt = rt(p.dt)
    A = np.eye(NX, dtype=dtype) + dt * np.swapaxes(fx, -1, -2).astype(dtype)
    B = dt * np.swapaxes(fu, -1, -2).astype(dtype)
    return A, B


def stage_cost(p, x, u, xg, dtype=np.float64):
    """dt/2 [(x - xg)' Q (x - xg) + (u - uh)' R (u - uh)] per knot, from the stored arrays x[..., 12], u[..., 4]"""
    c = Consts(p, dtype)
    dx, du = np.asarray(x, dtype) - np.asarray(xg, dtype), np.asarray(u, dtype) - c.uh
    return c.dt / 2 * ((c.q * dx * dx).sum(-1) + (c.r * du * du).sum(-1))


def terminal_cost(p, x, xg, dtype=np.float64):
    c = Consts(p, dtype)
    dx = np.asarray(x, dtype) - np.asarray(xg, dtype)
    return (c.qf * dx * dx).sum(-1) / 2


def total_cost(p, X, U, xg, dtype=np.float64):
    """cost of stored X[B, N+1, 12], U[B, N, 4]"""
    xg = np.asarray(xg, dtype)[:, None, :]
    return stage_cost(p, X[:, :-1], U, xg, dtype).sum(-1) + terminal_cost(p, X[:, -1], xg[:, 0], dtype)


def next_reg(reg, step, fp_failed, bp_failed):
    """the regulariser schedule, elementwise: failure +1, full step -1, step > 3 +1, clamped to 0..24"""
    reg, step = np.asarray(reg, np.int64), np.asarray(step, np.int64)
    failed = (np.asarray(fp_failed) != 0) | (np.asarray(bp_failed) != 0)
    d = np.where(failed, 1, np.where(step == 0, -1, np.where(step > 3, 1, 0)))
    return np.clip(reg + d, 0, REG_MAX)


def backward(p, X, U, xg, reg, store, dtype=LD, aux=None):
    """One backward sweep over X[B, N+1, 12], U[B, N, 4] with regulariser index reg[B].  Gains from Quu + lam I,
    lam = reg_base^reg - 1; value update with the unregularised Quu and the unrounded gains, symmetrised.
    Returns K[B, N, 4, 12], kf[B, N, 4] rounded to `store`, ok[B], and piv[B]: the smallest LLT pivot met, as a
    fraction of its diagonal entry (up to and including a failing one; inf where the diagonal itself is <= 0, when
    the failure holds exactly whatever the rounding).  aux (a dict) receives "kf_scale"[B]: the largest entry over the
    knots of |(Quu + lam I)^-1| (|l_u| + |B|' |V_x|), the size of the terms kf is the sum of (kf itself cancels to
    rounding noise at an optimum, so its own magnitude is no scale for its error)."""
    c = Consts(p, dtype)
    kf_scale = np.zeros(np.asarray(X).shape[0], dtype)
    X, U, xg = np.asarray(X, dtype), np.asarray(U, dtype), np.asarray(xg, dtype)
    Bn, N = X.shape[0], U.shape[1]
    lam = c.reg_base ** np.asarray(reg, np.int64).astype(dtype) - 1
    V = np.broadcast_to(np.diag(c.qf), (Bn, NX, NX)).copy()
    Vx = c.qf * (X[:, N] - xg)
    ok, piv = np.ones(Bn, bool), np.full(Bn, np.inf)
    K, kf = np.zeros((Bn, N, NU, NX), dtype), np.zeros((Bn, N, NU), dtype)
    T = lambda M: np.swapaxes(M, -1, -2)
    with np.errstate(all="ignore"):
        for k in range(N - 1, -1, -1):
            A, Bm = jacobians(p, X[:, k], U[:, k], dtype)
            Qx = c.dt * c.q * (X[:, k] - xg) + np.matmul(T(A), Vx[..., None])[..., 0]
            Qu = c.dt * c.r * (U[:, k] - c.uh) + np.matmul(T(Bm), Vx[..., None])[..., 0]
            VA = np.matmul(V, A)
            Qxx = np.matmul(T(A), VA) + np.diag(c.dt * c.q)
            Qux = np.matmul(T(Bm), VA)
            Quu = np.matmul(T(Bm), np.matmul(V, Bm)) + np.diag(c.dt * c.r)
            M = Quu + lam[:, None, None] * np.eye(NU, dtype=dtype)
            L = np.zeros((Bn, NU, NU), dtype)
            for j in range(NU):
                d = M[:, j, j] - (L[:, j, :j] ** 2).sum(-1)
                frac = np.where(M[:, j, j] > 0, np.abs(d / M[:, j, j]), np.inf).astype(np.float64)
                piv = np.where(ok, np.minimum(piv, frac), piv)
                bad = ~(d > 0)
                ok = ok & ~bad
                dj = np.sqrt(np.where(bad, 1, d))
                L[:, j, j] = dj
                if j + 1 < NU:
                    L[:, j + 1:, j] = (M[:, j + 1:, j] - np.matmul(L[:, j + 1:, :j], L[:, j, :j, None])[..., 0]) / dj[:, None]
            rhs = np.concatenate([Qu[:, :, None], Qux, np.broadcast_to(np.eye(NU, dtype=dtype), (Bn, NU, NU))], axis=2)   # [B, 4, 13 + 4]
            y = np.zeros_like(rhs)
            for i in range(NU):
                y[:, i] = (rhs[:, i] - np.matmul(L[:, i, None, :i], y[:, :i])[:, 0]) / L[:, i, i, None]
            z = np.zeros_like(rhs)
            for i in range(NU - 1, -1, -1):
                z[:, i] = (y[:, i] - np.matmul(T(L)[:, i, None, i + 1:], z[:, i + 1:])[:, 0]) / L[:, i, i, None]
            kk, Kk = -z[:, :, 0], -z[:, :, 1:1 + NX]
            qu_abs = np.abs(c.dt * c.r * (U[:, k] - c.uh)) + np.matmul(np.abs(T(Bm)), np.abs(Vx)[..., None])[..., 0]
            kf_scale = np.maximum(kf_scale, np.matmul(np.abs(z[:, :, 1 + NX:]), qu_abs[..., None])[..., 0].max(-1))
            K[:, k], kf[:, k] = rs(Kk, store, dtype), rs(kk, store, dtype)
            Vx = Qx + np.matmul(T(Kk), (np.matmul(Quu, kk[..., None])[..., 0] + Qu)[..., None])[..., 0] \
                + np.matmul(T(Qux), kk[..., None])[..., 0]
            Vn = Qxx + np.matmul(T(Kk), np.matmul(Quu, Kk)) + np.matmul(T(Kk), Qux) + np.matmul(T(Qux), Kk)
            V = (Vn + T(Vn)) / 2
    if aux is not None:
        aux["kf_scale"] = kf_scale
    return K, kf, ok, piv


def backward_with_retry(p, X, U, xg, reg, step, fp_failed, bp_failed, store, dtype=LD, aux=None):
    """The schedule, then the sweep; a failed LLT sets bp_failed and goes round again (at most 30 retries).
    Returns K, kf, reg[B], bp_failed[B], piv[B] (smallest pivot fraction over every attempt), retries[B]."""
    X, U, xg = np.asarray(X), np.asarray(U), np.asarray(xg)
    Bn, N = X.shape[0], U.shape[1]
    reg, step = np.array(reg, np.int64), np.asarray(step, np.int64)
    fp, bp = np.array(fp_failed, np.int64), np.array(bp_failed, np.int64)
    K, kf = np.zeros((Bn, N, NU, NX), dtype), np.zeros((Bn, N, NU), dtype)
    piv, retries = np.full(Bn, np.inf), np.zeros(Bn, np.int64)
    todo = np.arange(Bn)
    for attempt in range(MAX_RETRIES + 1):
        reg[todo] = next_reg(reg[todo], step[todo], fp[todo], bp[todo])
        a = {}
        Kt, kt, ok, pv = backward(p, X[todo], U[todo], xg[todo], reg[todo], store, dtype, a)
        K[todo], kf[todo] = Kt, kt
        if aux is not None:
            aux.setdefault("kf_scale", np.zeros(Bn, dtype))[todo] = a["kf_scale"]
        piv[todo] = np.minimum(piv[todo], pv)
        bp[todo] = np.where(ok, 0, 1)
        todo = todo[~ok]
        if todo.size == 0:
            break
        if attempt < MAX_RETRIES:
            retries[todo] += 1
    return K, kf, reg, bp, piv, retries


def forward_trial(p, X, U, K, kf, alpha, xg, store, dtype=np.float64):
    """One roll-out with step size alpha (scalar, or an array that broadcasts against the batch axes of X, e.g.
    alpha[11, 1] against X[B, ...] for all trials at once).  Returns Xn, Un (values of the storage type, held in
    `dtype`) and the cost accumulated in `dtype`."""
    c = Consts(p, dtype)
    X, U, K, kf, xg = (np.asarray(a, dtype) for a in (X, U, K, kf, xg))
    alpha = np.asarray(alpha, dtype)
    N = U.shape[-2]
    lead = np.broadcast_shapes(alpha.shape, X.shape[:-2])
    Xn, Un = np.zeros(lead + (N + 1, NX), dtype), np.zeros(lead + (N, NU), dtype)
    x = np.broadcast_to(X[..., 0, :], lead + (NX,))
    cost = np.zeros(lead, dtype)
    with np.errstate(all="ignore"):
        for k in range(N):
            Xn[..., k, :] = x
            fb = np.matmul(K[..., k, :, :], (x - X[..., k, :])[..., None])[..., 0]
            u = rs(U[..., k, :] + alpha[..., None] * kf[..., k, :] + fb, store, dtype)
            Un[..., k, :] = u
            cost = cost + stage_cost(p, x, u, xg, dtype)
            x = rs(x + c.dt * dynamics(p, x, u, dtype), store, dtype)
        Xn[..., N, :] = x
        cost = cost + terminal_cost(p, x, xg, dtype)
    return Xn, Un, cost


ALPHAS = 0.5 ** np.arange(N_STEPS)


def trial_costs(p, X, U, K, kf, xg, store, dtype=np.float64):
    """all 11 trials of a batch at once: Xn[11, B, N+1, 12], Un[11, B, N, 4], cost[11, B]"""
    return forward_trial(p, X, U, K, kf, ALPHAS[:, None], xg, store, dtype)


def begin(p, x0, xg, N, store, dtype=np.float64):
    """initial roll from the hover input, rounded like every other roll-out; returns the solver state (a dict)"""
    c = Consts(p, dtype)
    x0, xg = rs(np.atleast_2d(x0), store, dtype), rs(np.atleast_2d(xg), store, dtype)
    Bn = x0.shape[0]
    X, U = np.zeros((Bn, N + 1, NX), dtype), np.zeros((Bn, N, NU), dtype)
    U[:] = rs(c.uh, store, dtype)
    x, cost = x0, np.zeros(Bn, dtype)
    for k in range(N):
        X[:, k] = x
        cost = cost + stage_cost(p, x, U[:, k], xg, dtype)
        x = rs(x + c.dt * dynamics(p, x, U[:, k], dtype), store, dtype)
    X[:, N] = x
    cost = cost + terminal_cost(p, x, xg, dtype)
    z = lambda: np.zeros(Bn, np.int64)
    return dict(p=p, N=N, store=store, dtype=dtype, xg=xg, x=X, u=U, K=np.zeros((Bn, N, NU, NX), dtype),
                kf=np.zeros((Bn, N, NU), dtype), cost=cost, reg=z(), step=z(), fp_failed=z(), bp_failed=z(), iter=z(),
                done=z(), fwd_passes=z())


def iterate(s, n=1):
    """n trips of the outer loop on the state of `begin`, in place; returns done[B]"""
    p, store, dtype = s["p"], s["store"], s["dtype"]
    for _ in range(n):
        s["done"] = np.where((s["done"] != 0) | (s["iter"] >= p.iter_max), 1, 0)
        act = np.flatnonzero(s["done"] == 0)
        if act.size == 0:
            break
        K, kf, reg, bp, _, _ = backward_with_retry(p, s["x"][act], s["u"][act], s["xg"][act], s["reg"][act], s["step"][act],
                                                   s["fp_failed"][act], s["bp_failed"][act], store, dtype)
        s["K"][act], s["kf"][act], s["reg"][act], s["bp_failed"][act] = K, kf, reg, bp
        Xn, Un, cost = trial_costs(p, s["x"][act], s["u"][act], K, kf, s["xg"][act], store, dtype)
        prev = s["cost"][act]
        acc = cost < prev                                       # NaN fails the comparison and is rejected
        any_acc, first = acc.any(0), acc.argmax(0)
        j = np.arange(act.size)
        s["x"][act] = np.where(any_acc[:, None, None], Xn[first, j], s["x"][act])
        s["u"][act] = np.where(any_acc[:, None, None], Un[first, j], s["u"][act])
        s["cost"][act] = np.where(any_acc, cost[first, j], prev)
        s["step"][act] = np.where(any_acc, first, s["step"][act])
        s["fp_failed"][act] = np.where(any_acc, 0, 1)
        s["fwd_passes"][act] += 1
        s["iter"][act] += 1
        conv = (not p.fixed_iters) & any_acc & (prev - s["cost"][act] <= dtype(p.tol) * prev)
        s["done"][act] = np.where(conv | (s["iter"][act] >= p.iter_max), 1, 0)
    return s["done"]


SCALARS = ("cost", "reg", "step", "fp_failed", "bp_failed", "iter", "done", "fwd_passes")


def get(s):
    out = {k: np.array(s[k]).astype(s["store"]) for k in ("x", "u", "K", "kf")}
    out.update({k: np.array(s[k], np.float64) for k in SCALARS})
    return out


def solve(p, x0, xg, N, store=np.float64, dtype=np.float64):
    s = begin(p, x0, xg, N, store, dtype)
    iterate(s, p.iter_max)
    g = get(s)
    return dict(cost=g["cost"], iters=g["fwd_passes"].astype(np.int32), x=g["x"], u=g["u"])


class Stepper:
    """the stepper protocol of tests/quad_pass_lib.py (begin at construction, iterate, get) on the restatement"""

    def __init__(self, params, N, x0, xg, store=np.float64, dtype=np.float64):
        self.s = begin(params, x0, xg, N, store, dtype)

    def iterate(self, n=1):
        return iterate(self.s, n)

    def get(self):
        return get(self.s)

    def close(self):
        pass
