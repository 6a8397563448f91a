"""The C-ABI of the label model (include/direct_quad.h) on the paths no other test takes: a reused handle with
batch < max_batch, device-memory arguments on a caller's stream with every combination of NULL outputs (the path
bench.py measures), iter_max = 0, N = 1, and every DIRECT_ERR_INVALID return.  Every invalid call is rejected on the
host before anything is launched, and the handle stays usable."""
import ctypes as C
import itertools

import numpy as np
import pytest

from direct_amd import abi, quad
from oracle import quadapi
from tests import quad_pass_lib as L

pytestmark = pytest.mark.gpu

STORES = (np.float64, np.float32)


def _same(a, b):
    for k in ("cost", "iters", "x", "u"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_reused_handle_with_a_smaller_batch_equals_a_fresh_one(built, store):
    N = 40
    p1 = quad.default_params()
    a0, ag = quad.label_problems(64, seed=1000)
    p2 = quad.default_params(inertia=(C.c_double * 3)(*L.S2_INERTIA), q_ang=2.0, iter_max=9)
    b0, bg = L.s2_problems(5, 2140)
    h = quad.QuadSolver(64, N, store)
    first = h.solve(p1, a0, ag)
    small = h.solve(p2, b0, bg)
    fresh = quad.QuadSolver(5, N, store)
    want = fresh.solve(p2, b0, bg)
    _same(small, want)
    assert small["x"].shape == (5, N + 1, 12) and (small["iters"] > 0).all()
    # the stepwise interface on the reused handle: five trajectories, not sixty-four
    h.begin(p2, b0, bg); fresh.begin(p2, b0, bg)
    h.iterate(2); fresh.iterate(2)
    g, w = h.get(), fresh.get()
    for k in g:
        assert g[k].shape[0] == 5 and np.array_equal(g[k], w[k]), k
    _same(h.solve(p1, a0, ag), first)                     # and back
    h.close(); fresh.close()


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_device_memory_on_a_callers_stream_with_every_null_output(built, store):
    import torch
    dev = torch.device("cuda", 0)
    B, N = 8, 100
    p = quad.default_params(iter_max=10, fixed_iters=1) if store == np.float32 else quad.default_params()
    x0, xg = quad.label_problems(B, seed=1000)
    host = quad.QuadSolver(B, N, store)
    want = host.solve(p, x0, xg)
    host.close()
    td = torch.float64 if store == np.float64 else torch.float32
    stream = torch.cuda.Stream(device=dev)
    q = quad.QuadSolver(B, N, store)
    q.set_stream(stream.cuda_stream)
    tx0, txg = torch.from_numpy(x0.astype(store)).to(dev), torch.from_numpy(xg.astype(store)).to(dev)
    torch.cuda.synchronize()
    lib = quad._lib()
    for mask in itertools.product((0, 1), repeat=4):
        out = dict(cost=torch.full((B,), -1.0, dtype=td, device=dev), iters=torch.full((B,), -1, dtype=torch.int32, device=dev),
                   x=torch.full((B, N + 1, 12), -1.0, dtype=td, device=dev), u=torch.full((B, N, 4), -1.0, dtype=td, device=dev))
        torch.cuda.synchronize()
        ptr = [C.c_void_p(out[k].data_ptr()) if m else None for k, m in zip(("cost", "iters", "x", "u"), mask)]
        st = lib.direct_quad_solve_batch(q.h, C.addressof(p), B, abi.MEM_DEVICE, C.c_void_p(tx0.data_ptr()), C.c_void_p(txg.data_ptr()), *ptr)
        assert st == abi.DIRECT_OK, lib.direct_quad_last_error()
        stream.synchronize()
        for k, m in zip(("cost", "iters", "x", "u"), mask):
            got = out[k].cpu().numpy()
            if m:
                assert np.array_equal(got, want[k]), (mask, k)
            else:
                assert (got == -1).all(), (mask, k)           # a NULL output is not written through some other pointer
    assert q.last_kernel_ms() > 0
    q.set_stream(None)                                        # back on the default stream: same result through host memory
    _same(q.solve(p, x0, xg), want)
    q.close()


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_iter_max_zero_returns_the_begin_roll(built, store):
    N = 20
    x0, xg = quad.label_problems(3, seed=1000)
    q = quad.QuadSolver(3, N, store)
    out = q.solve(quad.default_params(iter_max=0), x0, xg)
    q.begin(quad.default_params(), x0, xg)
    g = q.get()
    assert (out["iters"] == 0).all()
    assert np.array_equal(out["x"], g["x"]) and np.array_equal(out["u"], g["u"]) and np.array_equal(out["cost"], g["cost"].astype(store))
    assert np.array_equal(out["u"], np.broadcast_to(np.array([0.98 * 9.81, 0, 0, 0]).astype(store), out["u"].shape))
    q.close()


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_a_single_knot(built, store):
    p = quad.default_params(inertia=(C.c_double * 3)(*L.S2_INERTIA))
    x0, xg = (a.astype(store).astype(np.float64) for a in L.s2_problems(6, 2101))
    q = quad.QuadSolver(6, 1, store)
    out = q.solve(p, x0, xg)
    q.close()
    r = quadapi.solve_batch(p, 1, x0, xg)
    assert out["x"].shape == (6, 2, 12) and out["u"].shape == (6, 1, 4)
    assert np.array_equal(out["x"][:, 0], x0.astype(store))
    if store == np.float64:                                   # whole-solve tolerances of tests/test_gpu_quad.py
        assert (np.abs(out["cost"] - r["cost"]) <= 1e-9 * r["cost"]).all()
        assert np.abs(out["x"] - r["x"]).max() < 1e-7 and np.abs(out["u"] - r["u"]).max() < 1e-6
    else:                                                     # float storage: cost 1e-3 as there; one Euler step from a float u
        assert (np.abs(out["cost"] - r["cost"]) <= 1e-3 * r["cost"]).all()
        assert np.abs(out["x"] - r["x"]).max() < 1e-5 * np.abs(r["x"]).max() and np.abs(out["u"] - r["u"]).max() < 1e-5 * np.abs(r["u"]).max()


def test_invalid_calls_are_rejected_and_leave_the_handle_usable(built):
    lib = quad._lib()
    N = 10
    x0, xg = quad.label_problems(4, seed=1000)
    q = quad.QuadSolver(4, N, np.float64)
    good = quad.default_params()
    buf = np.zeros(8)

    def begin(p, batch):
        return lib.direct_quad_begin(q.h, C.addressof(p) if p is not None else None, batch, abi.MEM_HOST, x0.ctypes.data, xg.ctypes.data)

    # before begin
    assert lib.direct_quad_iterate(q.h, 1) == abi.DIRECT_ERR_INVALID
    assert lib.direct_quad_get(q.h, None, None, None, None, buf.ctypes.data) == abi.DIRECT_ERR_INVALID
    assert lib.direct_quad_last_kernel_ms(q.h, buf.ctypes.data) == abi.DIRECT_ERR_INVALID
    assert lib.direct_quad_last_error()
    bad = [("batch > max_batch", good, 5), ("batch = 0", good, 0), ("mass 0", quad.default_params(mass=0.0), 4),
           ("zero inertia entry", quad.default_params(inertia=(C.c_double * 3)(2.64e-3, 0.0, 4.96e-3)), 4),
           ("reg_base 1", quad.default_params(reg_base=1.0), 4), ("iter_max -1", quad.default_params(iter_max=-1), 4),
           ("NULL params", None, 4)]
    for what, p, batch in bad:
        assert begin(p, batch) == abi.DIRECT_ERR_INVALID, what
        assert lib.direct_quad_iterate(q.h, 1) == abi.DIRECT_ERR_INVALID, what       # still not begun
    cost = np.zeros(4)
    for what, p, batch in bad:
        st = lib.direct_quad_solve_batch(q.h, C.addressof(p) if p is not None else None, batch, abi.MEM_HOST, x0.ctypes.data, xg.ctypes.data,
                                         cost.ctypes.data, None, None, None)
        assert st == abi.DIRECT_ERR_INVALID, what
    assert (cost == 0).all()
    want = quadapi.solve_batch(good, N, x0, xg)
    out = q.solve(good, x0, xg)                               # usable afterwards
    assert np.array_equal(out["iters"], want["iters"]) and (np.abs(out["cost"] - want["cost"]) <= 1e-9 * want["cost"]).all()
    for what, p, batch in bad:                                # and a rejected call after a good one changes nothing
        assert begin(p, batch) == abi.DIRECT_ERR_INVALID, what
    _same(q.solve(good, x0, xg), out)
    q.close()


def test_create_rejects_bad_arguments(built):
    lib = quad._lib()
    h = C.c_void_p()
    for what, args in (("dtype", (7, 0, 4, 10)), ("device -1", (abi.F64, -1, 4, 10)), ("device out of range", (abi.F64, 4096, 4, 10)),
                       ("max_batch 0", (abi.F64, 0, 0, 10)), ("max_batch -3", (abi.F32, 0, -3, 10)), ("n_knots 0", (abi.F32, 0, 4, 0)),
                       ("n_knots -1", (abi.F64, 0, 4, -1))):
        assert lib.direct_quad_create(*args, C.addressof(h)) == abi.DIRECT_ERR_INVALID, what
        assert not h.value
    assert lib.direct_quad_create(abi.F64, 0, 4, 10, None) == abi.DIRECT_ERR_INVALID
    assert lib.direct_quad_destroy(None) == abi.DIRECT_OK
