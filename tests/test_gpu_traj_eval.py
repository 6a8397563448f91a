"""direct_traj_eval_batch on the device (k_eval_starts + k_eval) against the NumPy restatement of its contract
(tests/traj_eval_lib.py), against k_sample at its own sample times and against the solver's jerk cost.

Bounds: double storage: pos / vel / acc within 1e-12 of the row's largest value, jerk / snap within 1e-9.  Float storage:
each output within one float ulp of the double restatement of the same float inputs, or within 1e-12 of the row maximum."""
import os

import numpy as np
import pytest

from direct_amd import abi, problems, solver
from tests import helpers
from tests import traj_eval_lib as L

pytestmark = pytest.mark.gpu
ALL = ("t_total", "seg", "pos", "vel", "acc", "jerk", "snap", "state")
SENTINEL = 7.25


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    return torch


def golden(name):
    return np.load(os.path.join(helpers.GOLDEN_DIR, name + ".npz"))


def check(d, r, dtype, rows=None):
    """device result d against restatement r (of the same rounded inputs)"""
    rows = range(len(r["status"])) if rows is None else rows
    assert np.array_equal(d["status"], r["status"])
    if "seg" in d:
        assert np.array_equal(d["seg"], r["seg"])
    if "t_total" in d:
        assert np.array_equal(d["t_total"].astype(np.float64), r["t_total"].astype(dtype).astype(np.float64))
    names = [n for n in L.NAMES + ("state",) if n in d]
    for name in names:
        tol = 1e-9 if name in ("jerk", "snap") and dtype == np.float64 else 1e-12
        for b in rows:
            a, e = d[name][b].astype(np.float64), r[name][b]
            nan = np.isnan(e)
            assert np.array_equal(np.isnan(a), nan), (name, b)
            if not (~nan).any():
                continue
            err = np.abs(a - e)[~nan]
            scale = np.abs(e[~nan]).max()
            if dtype == np.float64:
                assert err.max() <= tol * scale + 1e-300, (name, b, err.max() / scale)
            else:
                ulp = np.spacing(np.abs(e[~nan]).astype(np.float32)).astype(np.float64)
                assert ((err <= ulp) | (err <= 1e-12 * scale)).all(), (name, b, (err / ulp).max())


def run_device(s, dtype, n_seg, T, times=None, t0=0.0, dt=0.0, m=None, n_query=None, outputs=ALL, **src):
    """the same call through device-resident torch tensors on the handle's stream; outputs pre-filled with a sentinel"""
    torch = _torch()
    dev = torch.device("cuda:0")
    s.set_stream(torch.cuda.current_stream().cuda_stream)
    td = torch.float64 if dtype == np.float64 else torch.float32
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dt_)).to(dev)
    B, nm = np.asarray(T).shape
    keep = dict(n_seg=up(n_seg, np.int32), T=up(T, dtype))
    cin, cout = abi.EvalIn(), abi.EvalOut()
    for k, v in src.items():
        keep[k] = up(v, dtype)
    if times is not None:
        keep["t"] = up(times, dtype)
        m = times.shape[1]
    if n_query is not None:
        keep["n_query"] = up(n_query, np.int32)
    cin.batch, cin.n_seg_max, cin.m_max, cin.mem, cin.t0, cin.dt = B, nm, m, abi.MEM_DEVICE, t0, dt
    for k, v in keep.items():
        setattr(cin, k, v.data_ptr())
    shapes = dict(t_total=(B,), seg=(B, m), state=(B, m, 9))
    o = {"status": torch.full((B,), -7, dtype=torch.int32, device=dev)}
    for k in outputs:
        o[k] = (torch.full(shapes[k], -7, dtype=torch.int32, device=dev) if k == "seg"
                else torch.full(shapes.get(k, (B, m, 3)), SENTINEL, dtype=td, device=dev))
    for k, v in o.items():
        setattr(cout, k, v.data_ptr())
    s.evaluate_device(cin, cout)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def mixed_times(n_seg, T, m, seed):
    """sorted random times over [-0.5, S_n + 0.5] with every segment start written over every 7th (so the first chunk spans
    all segments: the per-query path), and a NaN"""
    rng = np.random.default_rng(seed)
    B = len(n_seg)
    t = np.zeros((B, m))
    for b in range(B):
        S = L.starts(T[b], int(n_seg[b]))
        x = np.sort(rng.uniform(-0.5, S[-1] + 0.5, m))
        x[::7][:len(S)] = S[:len(x[::7])]
        x[5] = np.nan
        t[b] = x
    return t


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("src", ["bez", "poly"])
@pytest.mark.parametrize("grid", [False, True])
def test_kernel_against_the_restatement(built, dtype, mem, src, grid):
    for case in ("corridor_n8", "config1_n50"):
        g = golden(case)
        n_seg = g["n_seg"]
        T, coef = g["p1_T"].astype(dtype), g["p1_" + src].astype(dtype)
        B, nm = T.shape
        n_query = np.arange(B, dtype=np.int32) * 97 + 600
        kw = dict(t0=-0.05, dt=0.013, m=777) if grid else dict(times=mixed_times(n_seg, T.astype(np.float64), 700, 3).astype(dtype))
        r = L.evaluate(n_seg, T, n_query=n_query, **kw, **{src: coef})
        s = solver.DdpSolver(B, nm, 6, dtype)
        if mem == "host":
            d = s.evaluate(n_seg, T, n_query=n_query, outputs=ALL, **kw, **{src: coef})
        else:
            d = run_device(s, dtype, n_seg, T, n_query=n_query, **kw, **{src: coef})
            m = d["seg"].shape[1]
            for b in range(B):   # entries past n_query are left untouched in device memory
                past = slice(min(int(n_query[b]), m), m)
                assert (d["seg"][b, past] == -7).all() and (d["pos"][b, past] == SENTINEL).all()
                assert (d["state"][b, past] == SENTINEL).all() and (d["snap"][b, past] == SENTINEL).all()
                d["seg"][b, past] = 0
                for k in L.NAMES + ("state",):
                    d[k][b, past] = 0
        check(d, r, dtype)
        # state is pos, vel, acc interleaved, bit for bit
        assert np.array_equal(d["state"], np.concatenate([d["pos"], d["vel"], d["acc"]], -1), equal_nan=True)
        assert s.eval_last_ms() > 0
        s.close()


def test_against_k_sample_on_gpu_plans(built):
    """k_sample's pos / vel / acc are the plan at S_i + k step T_i (its own sample times)."""
    batch = problems.make_batch("free", 64, 20, seed=31)
    s = solver.DdpSolver(64, 20, batch.p_max, np.float64)
    _, g1 = s.plan(abi.phase0_params(), abi.phase1_params(iter_max=20, fixed_iters=1), batch)
    dt, cap = 0.05, 2048
    o = s.sample(batch.n_seg, g1.bez, g1.T, dt, cap)
    t = np.zeros((64, cap))
    for b in range(64):
        S = L.starts(g1.T[b], int(batch.n_seg[b]))
        for i in range(int(batch.n_seg[b])):
            first = o["seg_first"][b, i]
            last = o["seg_first"][b, i + 1] if i + 1 < batch.n_seg[b] else o["count"][b]
            k = np.arange(last - first)
            t[b, first:last] = S[i] + (k * (dt / g1.T[b, i])) * g1.T[b, i]
    d = s.evaluate(batch.n_seg, g1.T, bez=g1.bez, times=t, outputs=("pos", "vel", "acc"))
    for b in range(64):
        c = int(o["count"][b])
        assert c <= cap
        for f in ("pos", "vel", "acc"):
            assert helpers.rel(d[f][b, :c], o[f][b, :c]) < 1e-12, (b, f)
    s.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jerk_cost_witness_on_device(built, dtype):
    """Gauss-Legendre quadrature of the kernel's jerk equals the same plan's jerk_cost output."""
    batch = problems.make_batch("corridor", 32, 12, seed=5)
    s = solver.DdpSolver(32, 12, batch.p_max, dtype)
    _, g1 = s.plan(abi.phase0_params(), abi.phase1_params(), batch)
    ok = g1.rtn >= 0
    assert ok.mean() > 0.8
    t, w = L.gauss_times(batch.n_seg, g1.T.astype(np.float64))
    for src, tol in (("poly", 1e-12), ("bez", 1e-9)):
        d = s.evaluate(batch.n_seg, g1.T, times=np.nan_to_num(t), outputs=("jerk",), **{src: getattr(g1, src)})
        jc = L.jerk_cost(d["jerk"], w)
        if dtype == np.float64:
            assert np.abs(jc / g1.jerk_cost - 1)[ok].max() < tol, src
        else:   # the restatement of the same float inputs, and the float jerk_cost to float rounding
            r = L.evaluate(batch.n_seg, g1.T, times=np.nan_to_num(t), **{src: getattr(g1, src)})
            assert np.abs(jc / L.jerk_cost(r["jerk"], w) - 1)[ok].max() < 1e-5, src
    s.close()


def test_invalid_rows_leave_valid_rows_bit_identical(built):
    g = golden("corridor_n8")
    n_seg, T, bez = g["n_seg"].copy(), g["p1_T"].copy(), g["p1_bez"]
    t = mixed_times(n_seg, T, 300, 9)
    s = solver.DdpSolver(6, T.shape[1], 6, np.float64)
    want = s.evaluate(n_seg, T, bez=bez, times=t, outputs=ALL)
    nn = np.concatenate([n_seg, [0, T.shape[1] + 1, n_seg[0]]]).astype(np.int32)
    TT = np.concatenate([T, T[:1], T[:1], T[:1]])
    TT[5, 2] = -1.0
    bb = np.concatenate([bez, bez[:1], bez[:1], bez[:1]])
    tt = np.concatenate([t, t[:1], t[:1], t[:1]])
    d = s.evaluate(nn, TT, bez=bb, times=tt, outputs=ALL)
    assert list(d["status"]) == [0, 0, 0, -1, -1, -1]
    for k in ALL:
        assert np.array_equal(d[k][:3], want[k], equal_nan=True), k
        assert (d[k][3:] == (-1 if k == "seg" else 0)).all(), k
    s.close()


@pytest.mark.parametrize("n", [300, 1000, 1500])
@pytest.mark.parametrize("src", ["bez", "poly"])
def test_long_rows(built, n, src):
    """Rows of many segments: S in LDS (n < 1024) or in the workspace (1500); chunks spanning more segments than the LDS
    slots (explicit unsorted times, and a coarse grid) take the per-query path."""
    rng = np.random.default_rng(n)
    B = 3
    T = rng.uniform(0.2, 1.5, (B, n))
    coef = rng.normal(0.0, 1.0, (B, n, 18))
    n_seg = np.array([n, n - 7, n // 2], np.int32)
    S_end = T.sum(1)
    times = rng.uniform(-1.0, S_end.max() + 1.0, (B, 2000))
    s = solver.DdpSolver(B, n, 6, np.float64)
    for kw in (dict(times=times), dict(t0=0.0, dt=0.01, m=3000), dict(t0=-0.1, dt=S_end.max() / 900, m=1000)):
        d = s.evaluate(n_seg, T, outputs=ALL, **kw, **{src: coef})
        check(d, L.evaluate(n_seg, T, **kw, **{src: coef}), np.float64)
    s.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_row_of_a_million_queries(built, dtype):
    batch = problems.make_batch("free", 1, 100, seed=77)
    s = solver.DdpSolver(1, 100, batch.p_max, dtype)
    _, g1 = s.plan(abi.phase0_params(), abi.phase1_params(iter_max=20, fixed_iters=1), batch)
    m = 1 << 20
    total = float(g1.T.astype(np.float64).sum())
    dt = total / (m - 1000)
    d = run_device(s, dtype, batch.n_seg, g1.T, t0=-0.01, dt=dt, m=m, poly=g1.poly,
                   outputs=("seg", "pos", "vel", "acc", "jerk", "snap"))
    idx = np.unique(np.concatenate([np.arange(0, m, 257), np.arange(m - 2000, m)]))
    r = L.evaluate(batch.n_seg, g1.T, poly=g1.poly, times=(-0.01 + idx * dt)[None])
    sub = {k: v[:, idx] for k, v in d.items() if k != "status"}
    sub["status"] = d["status"]
    check(sub, r, dtype)
    assert (d["seg"][0, -500:] == 99).all()   # past S_n: clamped into the last segment
    s.close()


def test_batches_past_the_16_bit_grid_dimension(built):
    """k_eval's grid is (chunks, batch) with batch in launches of at most 65535 rows: a batch of 70000 covers the split."""
    B = 70000
    rng = np.random.default_rng(11)
    n_seg = np.full(B, 2, np.int32)
    T = rng.uniform(0.5, 1.5, (B, 2))
    poly = rng.normal(0.0, 1.0, (B, 2, 18))
    n_seg[[3, 65534, 65535, 69999]] = 0          # invalid rows on both sides of the split
    times = rng.uniform(0.0, 3.0, (B, 1))
    s = solver.DdpSolver(1, 2, 6, np.float64)
    d = s.evaluate(n_seg, T, poly=poly, times=times, outputs=("t_total", "seg", "pos", "snap"))
    r = L.evaluate(n_seg, T, poly=poly, times=times)
    check(d, r, np.float64)
    assert (d["status"][[3, 65534, 65535, 69999]] == -1).all() and (d["status"] == 0).sum() == B - 4
    s.close()
