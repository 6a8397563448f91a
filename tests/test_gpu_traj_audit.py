"""direct_traj_audit_batch on the device (k_audit_starts, k_audit_items, k_audit_rows, k_audit_best of
direct_amd/csrc/traj_audit.h) against the g++ build of the same arithmetic (tests/traj_audit_harness.py), which
tests/test_traj_audit_restatement.py holds against the exact fixture.

Bounds.  Double storage: every output bit-identical to the CPU build (slowdown within 2 ulp: cbrt is within 1 ulp in each of
the two maths libraries, not correctly rounded).  Float storage: the double result of the float inputs, rounded to float
(slowdown within one float ulp).  Solved plans: the CPU build of the copied-back plans, the same way; independent of it, every
segment's peaks lie between 2000 dense samples and the control polygon's largest magnitude (tests/traj_audit_lib.py, sandwich,
within the 24 u F tolerance); and the audit's peaks are never below the sampler's maxima over samples."""
import os

import numpy as np
import pytest

from direct_amd import abi, problems, solver
from tests import helpers
from tests import traj_audit_harness as H
from tests import traj_audit_lib as L

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(helpers.GOLDEN_DIR, "audit_cases.npz"))
CASES = [str(c) for c in FIX["cases"]]
INTS = ("status", "c_where", "verdict", "best")
SENTINEL = 7.25
LIMITS = dict(max_vel=1.9, max_acc=1.4, max_jerk=3.4, clearance=0.02)


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    return torch


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("audit_math_gpu"))


def case(name, dtype):
    """the fixture's inputs in the storage type (float cases of the fixture hold float values already)"""
    c = L.fixture_case(FIX, name, helpers.GOLDEN_DIR)
    r = dict(n_seg=c["n_seg"], T=c["T"].astype(dtype), coef=c["coef"].astype(dtype), src=c["src"], n_planes=None, planes=None)
    if c["planes"] is not None:
        r["n_planes"], r["planes"] = c["n_planes"], c["planes"].astype(dtype)
    return r


def cpu(harness, c, on_norm=0, cost=None, rtn=None, limits=LIMITS):
    lim = (limits["max_vel"], limits["max_acc"], limits["max_jerk"], limits["clearance"])
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    return H.run(harness, c["n_seg"], f(c["T"]), f(c["coef"]), c["src"], c["n_planes"], f(c["planes"]), limits=lim, on_norm=on_norm,
                 cost=f(cost), rtn=rtn)


def outputs_for(c, cost):
    return [k for k in abi.AUDIT_OUTPUTS if not (k in ("cpeak", "c_where") and c["planes"] is None) and not (k == "best" and cost is None)]


def run_host(s, c, on_norm=0, cost=None, rtn=None, outputs=None, limits=LIMITS):
    return s.audit(c["n_seg"], c["T"], n_planes=c["n_planes"], planes=c["planes"], limit_on_norm=on_norm, cost=cost, rtn=rtn,
                   outputs=outputs, **limits, **{c["src"]: c["coef"]})


def run_device(s, dtype, c, on_norm=0, cost=None, rtn=None, outputs=None, limits=LIMITS):
    """the same call through device-resident torch tensors on the handle's stream; outputs pre-filled with a sentinel"""
    torch = _torch()
    dev = torch.device("cuda:0")
    s.set_stream(torch.cuda.current_stream().cuda_stream)
    td = torch.float64 if dtype == np.float64 else torch.float32
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(a, dt_)).to(dev)
    B, nm = c["T"].shape
    keep = dict(n_seg=up(c["n_seg"], np.int32), T=up(c["T"], dtype))
    keep[c["src"]] = up(c["coef"].reshape(B, nm, 18), dtype)
    cin, cout = abi.AuditIn(), abi.AuditOut()
    if c["planes"] is not None:
        keep["n_planes"], keep["planes"] = up(c["n_planes"], np.int32), up(c["planes"], dtype)
        cin.p_max = c["planes"].shape[2]
    if cost is not None:
        keep["cost"] = up(cost, dtype)
    if rtn is not None:
        keep["rtn"] = up(rtn, np.int32)
    cin.batch, cin.n_seg_max, cin.mem, cin.limit_on_norm = B, nm, abi.MEM_DEVICE, on_norm
    cin.max_vel, cin.max_acc, cin.max_jerk, cin.clearance = (limits[k] for k in ("max_vel", "max_acc", "max_jerk", "clearance"))
    for k, v in keep.items():
        setattr(cin, k, v.data_ptr())
    outputs = outputs_for(c, cost) if outputs is None else outputs
    shapes = dict(c_where=(B, 2), at=(B, 4), seg_peak=(B, nm, 4), gap=(B, 3), best=(1,))
    o = {"status": torch.full((B,), -7, dtype=torch.int32, device=dev)}
    for k in outputs:
        if k in INTS:
            o[k] = torch.full(shapes.get(k, (B,)), -7, dtype=torch.int64 if k == "best" else torch.int32, device=dev)
        else:
            o[k] = torch.full(shapes.get(k, (B,)), SENTINEL, dtype=td, device=dev)
    for k, v in o.items():
        setattr(cout, k, v.data_ptr())
    s.audit_device(cin, cout)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def same(d, r, dtype, n_seg=None, device=False):
    """device result d against the CPU build r of the same (rounded) inputs"""
    for k, v in d.items():
        want = r[k]
        if k in INTS:
            assert np.array_equal(v, want), k
            continue
        got = v.astype(np.float64)
        if k == "seg_peak" and device:     # entries past n_seg are left untouched in device memory
            for b, n in enumerate(n_seg):
                n = min(max(int(n), 0), v.shape[1])
                assert (got[b, n:] == SENTINEL).all(), (k, b)
                got[b, n:] = 0.0
        want = want.astype(dtype).astype(np.float64)
        if k == "slowdown":
            ulp = np.spacing(np.abs(want).astype(dtype)).astype(np.float64)
            assert (np.abs(got - want) <= (2 if dtype == np.float64 else 1) * ulp).all(), k
        else:
            assert np.array_equal(got, want), (k, np.abs(got - want).max())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mem", ["host", "device"])
def test_kernels_bit_identical_to_the_cpu_build(built, harness, dtype, mem):
    rng = np.random.default_rng(4)
    for name in CASES:
        if ("_f32_" in name) != (dtype == np.float32) and "synthetic" not in name and "invalid" not in name:
            continue
        c = case(name, dtype)
        B, nm = c["T"].shape
        cost = rng.uniform(1.0, 2.0, B).astype(dtype)
        rtn = rng.integers(-1, 2, B).astype(np.int32)
        s = solver.DdpSolver(B, nm, 6, dtype)
        for on_norm in (0, 1):
            r = cpu(harness, c, on_norm, cost, rtn)
            d = run_host(s, c, on_norm, cost, rtn) if mem == "host" else run_device(s, dtype, c, on_norm, cost, rtn)
            assert set(d) == set(outputs_for(c, cost)) | {"status"}
            same(d, r, dtype, c["n_seg"], mem == "device")
        assert s.audit_last_ms() > 0
        s.close()


def test_outputs_null_in_turn_and_nothing_else_written(built, harness):
    """every optional pointer NULL in turn: the others keep their bits; without cost, rtn, corridor and norms"""
    torch = _torch()
    c = case("corridor_n8_p1_f64_poly", np.float64)
    B, nm = c["T"].shape
    cost = np.linspace(2.0, 1.0, B)
    s = solver.DdpSolver(B, nm, 6, np.float64)
    full = run_device(s, np.float64, c, cost=cost)
    names = outputs_for(c, cost)
    for drop in names:
        d = run_device(s, np.float64, c, cost=cost, outputs=[k for k in names if k != drop])
        assert drop not in d
        for k, v in d.items():
            assert np.array_equal(v, full[k]), (drop, k)
    free = dict(c, n_planes=None, planes=None)
    d = run_device(s, np.float64, free, outputs=("vpeak", "apeak", "jpeak", "at", "seg_peak", "verdict"))   # no norm items run
    r = cpu(harness, free)
    same(d, {k: r[k] for k in d}, np.float64, c["n_seg"], True)
    assert (d["at"][:, 3] == 0).all() and (d["seg_peak"][:, :, 3][d["seg_peak"][:, :, 3] != SENTINEL] == 0).all()
    # the guard cells around a device output stay: seg_peak of a batch embedded in a larger buffer
    dev = torch.device("cuda:0")
    buf = torch.full((B + 2, 1), SENTINEL, dtype=torch.float64, device=dev)
    cin, cout = abi.AuditIn(), abi.AuditOut()
    keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (c["n_seg"].astype(np.int32), c["T"], c["coef"])]
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    cin.batch, cin.n_seg_max, cin.mem = B, nm, abi.MEM_DEVICE
    cin.n_seg, cin.T, cin.poly = (k.data_ptr() for k in keep)
    cout.status, cout.vpeak = st.data_ptr(), buf[1:].data_ptr()
    s.audit_device(cin, cout)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()[:, 0]
    assert got[0] == SENTINEL and got[-1] == SENTINEL and np.array_equal(got[1:B + 1], full["vpeak"])
    s.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_independent_of_the_launch_shape(built, dtype):
    """one call, two calls of halves, and permuted rows give identical rows and the corresponding best"""
    batch = problems.make_batch("corridor", 192, 20, seed=12)
    s = solver.DdpSolver(192, 20, batch.p_max, dtype)
    _, g1 = s.plan(abi.phase0_params(), abi.phase1_params(iter_max=30), batch)
    rows = np.arange(192)
    rows = rows[rows % 7 != 3]        # 164 rows: a wave of k_audit_items then straddles rows at other places than in the halves
    c = dict(n_seg=batch.n_seg[rows], T=g1.T[rows], coef=g1.poly[rows], src="poly", n_planes=batch.n_planes[rows],
             planes=batch.planes[rows].astype(dtype))
    cost, rtn = g1.cost[rows], g1.rtn[rows]
    free = run_device(s, dtype, c, outputs=("jpeak",), limits=dict(max_vel=0.0, max_acc=0.0, max_jerk=0.0, clearance=0.0))
    lim = dict(max_vel=2.0 * 1.02, max_acc=2.0 * 1.02, max_jerk=float(np.median(free["jpeak"])), clearance=0.0)   # about half the rows pass
    whole = run_device(s, dtype, c, cost=cost, rtn=rtn, limits=lim)
    assert (whole["status"] == 0).all()
    passing = (whole["verdict"] == 0) & (rtn >= 0)
    assert 0 < passing.sum() < len(rows)
    assert whole["best"][0] == L.best_row(cost, whole["verdict"], rtn)
    sel = lambda idx: {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    h = len(rows) // 2 + 5
    for idx in (np.arange(h), np.arange(h, len(rows)), np.random.default_rng(3).permutation(len(rows))):
        d = run_device(s, dtype, sel(idx), cost=cost[idx], rtn=rtn[idx], limits=lim)
        for k, v in d.items():
            if k != "best":
                assert np.array_equal(v, whole[k][idx]), k
        want = L.best_row(cost[idx], whole["verdict"][idx], rtn[idx])
        assert d["best"][0] == want and (want < 0 or cost[idx][want] == cost[idx][passing[idx]].min())
    s.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_end_to_end_on_solved_plans_in_device_memory(built, harness, dtype):
    """direct_ddp_plan_batch with device memory, then the audit on out.poly / out.T and the input planes without visiting the host"""
    torch = _torch()
    dev = torch.device("cuda:0")
    B, N = 256, 20
    batch = problems.make_batch("corridor", B, N, seed=21).astype(dtype)
    s = solver.DdpSolver(B, N, batch.p_max, dtype)
    s.set_stream(torch.cuda.current_stream().cuda_stream)
    td = torch.float64 if dtype == np.float64 else torch.float32
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    inp = {k: up(getattr(batch, k)) for k in ("n_seg", "x0", "xd", "T0", "n_planes", "planes", "seeds")}
    cin = abi.BatchIn()
    cin.batch, cin.n_seg_max, cin.p_max, cin.mem = B, N, batch.p_max, abi.MEM_DEVICE
    for k, v in inp.items():
        setattr(cin, k, v.data_ptr())
    res = dict(rtn=torch.zeros(B, dtype=torch.int32, device=dev), cost=torch.zeros(B, dtype=td, device=dev),
               bez=torch.zeros((B, N, 18), dtype=td, device=dev), poly=torch.zeros((B, N, 18), dtype=td, device=dev),
               T=torch.zeros((B, N), dtype=td, device=dev))
    cout = abi.BatchOut()
    cout.mem = abi.MEM_DEVICE
    for k, v in res.items():
        setattr(cout, k, v.data_ptr())
    p0, p1 = abi.phase0_params(), abi.phase1_params()
    s.plan_device(p0, p1, cin, None, cout)
    lim = dict(max_vel=2.0 * 1.001, max_acc=2.0 * 1.001, max_jerk=10.0, clearance=0.0)
    names = [k for k in abi.AUDIT_OUTPUTS]
    shapes = dict(c_where=(B, 2), at=(B, 4), seg_peak=(B, N, 4), gap=(B, 3), best=(1,))

    def audit(src):
        a, o = abi.AuditIn(), abi.AuditOut()
        a.batch, a.n_seg_max, a.p_max, a.mem = B, N, batch.p_max, abi.MEM_DEVICE
        a.n_seg, a.T, a.n_planes, a.planes = inp["n_seg"].data_ptr(), res["T"].data_ptr(), inp["n_planes"].data_ptr(), inp["planes"].data_ptr()
        setattr(a, src, res[src].data_ptr())
        a.cost, a.rtn = res["cost"].data_ptr(), res["rtn"].data_ptr()
        a.max_vel, a.max_acc, a.max_jerk, a.clearance = lim["max_vel"], lim["max_acc"], lim["max_jerk"], lim["clearance"]
        out = {"status": torch.zeros(B, dtype=torch.int32, device=dev)}
        for k in names:
            out[k] = torch.zeros(shapes.get(k, (B,)), dtype=(torch.int64 if k == "best" else torch.int32) if k in INTS else td, device=dev)
        for k, v in out.items():
            setattr(o, k, v.data_ptr())
        s.audit_device(a, o)          # enqueued behind the plan on the same stream: nothing has visited the host yet
        return out

    out_poly, out_bez = audit("poly"), audit("bez")
    torch.cuda.synchronize()
    d = {k: v.cpu().numpy() for k, v in out_poly.items()}
    db = {k: v.cpu().numpy() for k, v in out_bez.items()}
    host = {k: v.cpu().numpy() for k, v in res.items()}
    assert (d["status"] == 0).all() and (host["rtn"] >= 0).mean() > 0.8
    # the CPU build of the copied-back plans (held against the exact fixture by test_traj_audit_restatement): the same bits
    c = dict(n_seg=batch.n_seg, T=host["T"], coef=host["poly"], src="poly", n_planes=batch.n_planes, planes=batch.planes)
    r = cpu(harness, c, cost=host["cost"], rtn=host["rtn"], limits=lim)
    same(d, r, dtype, batch.n_seg)
    # independent of that build: the bracket that needs no oracle (dense samples <= peak + tol, peak <= control polygon + tol) on
    # every segment of the copied-back plans, for the double results that the device's outputs are the roundings of
    f64 = lambda x: np.asarray(x, np.float64)
    tol = L.tolerances(c["n_seg"], f64(c["T"]), f64(c["coef"]), "poly", c["n_planes"], f64(c["planes"]))
    L.sandwich(c["n_seg"], f64(c["T"]), f64(c["coef"]), "poly", r["seg_peak"], tol["seg_peak"], c["n_planes"], f64(c["planes"]))
    assert d["best"][0] == L.best_row(host["cost"], d["verdict"], host["rtn"])
    n_pass = int(((d["verdict"] == 0) & (host["rtn"] >= 0)).sum())
    assert 0 < n_pass
    print("rows passing the audit: %d of %d; verdict histogram %s" % (n_pass, B, np.unique(d["verdict"], return_counts=True)))
    # never below the sampler: from out.bez, the sampler's own input
    sm = s.sample(batch.n_seg, host["bez"], host["T"], 0.1, 4096, n_planes=batch.n_planes, planes=batch.planes)
    cb = dict(c, coef=host["bez"], src="bez")
    tb = L.tolerances(cb["n_seg"], cb["T"].astype(np.float64), cb["coef"].astype(np.float64), "bez", cb["n_planes"], cb["planes"].astype(np.float64))
    for f, g in (("vpeak", "vmax"), ("apeak", "amax"), ("cpeak", "cmax")):
        got, low = db[f].astype(np.float64), sm[g].astype(np.float64)
        slack = tb[f] + (np.spacing(np.abs(low).astype(np.float32)).astype(np.float64) if dtype == np.float32 else 0.0)
        assert (got >= low - slack).all(), (f, (low - got).max())
    s.close()


def test_batches_wider_than_one_launch_dimension_and_long_rows(built, harness):
    """70000 rows of 2 segments (k_audit_rows: one workgroup per row), and 3 rows of 700 segments (rows over many waves)"""
    rng = np.random.default_rng(8)
    for B, n in ((70000, 2), (3, 700)):
        n_seg = np.full(B, n, np.int32)
        n_seg[[1, B - 1]] = (0, n - 1)
        T = rng.uniform(0.5, 1.5, (B, n))
        poly = rng.normal(0.0, 1.0, (B, n, 18))
        c = dict(n_seg=n_seg, T=T, coef=poly, src="poly", n_planes=None, planes=None)
        cost = rng.uniform(1.0, 2.0, B)
        s = solver.DdpSolver(1, n, 6, np.float64)
        d = run_host(s, c, cost=cost, limits=dict(max_vel=4.0, max_acc=0.0, max_jerk=0.0, clearance=0.0))
        r = cpu(harness, c, cost=cost, limits=dict(max_vel=4.0, max_acc=0.0, max_jerk=0.0, clearance=0.0))
        same(d, r, np.float64)
        assert d["status"][1] == -1 and d["verdict"][1] == abi.AUDIT_INVALID and (d["status"] == 0).sum() == B - 1
        s.close()
