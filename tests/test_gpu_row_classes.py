"""Every row-slot class of the DDP kernels, iteration by iteration (tests/row_class_lib.py).

The kernels are instantiated for 2 .. 8, 10, 12 and 14 row slots of 64 per lane (direct_ddp.hip, rpl_class): a knot has
6 P + 55 constraint rows, and what changes with the class is the row-slot skipping of Wave::slot_on, the width of the
packed row descriptor (kRB), the reuse of descriptors across knots of equal plane count (pk_valid), the plane buffers
(kPMax, kNPL), the launch bounds and, for classes 2 .. 4 only, the sharing instantiations k_iterate_dyn<Real, R, true>.
Small ragged batches at the lowest and highest p_max of every class, knots at the slot boundaries
(helpers.with_edge_planes):
  * gains of one backward pass and four single outer iterations of both phases against the oracle (double storage) and
    against the lane-loop emulator of the same source (float storage: its distance to the oracle is storage rounding,
    up to 1e-3 at P = 128 in feasible mode, so the oracle check next to it is loose);
  * every launch form bit for bit at every class, both storage types;
  * one batch holding every class, on one class-14 launch and sorted into classes (DIRECT_DDP_CLASSES=1)."""
import numpy as np
import pytest

from direct_amd import abi, problems, solver
from tests import helpers, row_class_lib
from tests.emu import emuapi

pytestmark = pytest.mark.gpu
CLASS_TOP = (12, 22, 33, 44, 54, 65, 76, 97, 118, 128)   # the highest p_max of every class
FIELDS = ("rtn", "iter_used", "fwd_passes", "infeas_out", "line_failed_out", "cost", "costq", "opterr", "mu", "T", "poly", "bez")


def begun(params, batch, dtype):
    s = solver.DdpSolver(batch.batch, batch.n_seg_max, batch.p_max, dtype)
    s.begin(params, batch)
    return s


@pytest.mark.parametrize("p_max", row_class_lib.CLASS_EDGES)
def test_gains_of_one_backward_pass(built, p_max):
    """KU / KUU / KS / KY of the first backward sweep of both phases, double storage, against the oracle: 1e-10 (KY in
    infeasible mode only: in feasible mode there is no dual gain and the array is not written, include/direct_ddp.h).
    Measured: 1.2e-11 at most (class 14)."""
    batch = row_class_lib.edge_batch(p_max)
    for name, params, b in row_class_lib.phases(batch):
        s, o = begun(params, b, np.float64), row_class_lib.Oracle(params, b)
        s.backward()
        o.backward()
        gains = {}
        for f in (abi.FIELD_KU, abi.FIELD_KUU, abi.FIELD_KS) + ((abi.FIELD_KY,) if params.infeas else ()):
            gains[f] = row_class_lib.field_dev(s.get(f), o.get(f), b, f)
        row_class_lib.record("gains_f64", (p_max, name), {str(k): v for k, v in gains.items()})
        for f, d in gains.items():
            assert d < 1e-10, (name, f, d)
        assert (s.scalars()["bp_failed"] == 0).all()
        s.close()
        o.close()


@pytest.mark.parametrize("p_max", row_class_lib.CLASS_EDGES)
def test_stepped_iterates_double_storage(built, p_max):
    """four single outer iterations of both phases against the oracle: every discrete decision identical after each,
    X / U / S / Y (Y in infeasible mode) and the continuous scalars within 1e-10 per problem (opterr:
    row_class_lib.check_scalars).  Measured: fields 1.4e-11 at most (class 8), opterr 8.3e-10 (class 8, phase 1)."""
    batch = row_class_lib.edge_batch(p_max)
    for name, params, b in row_class_lib.phases(batch):
        s, o = begun(params, b, np.float64), row_class_lib.Oracle(params, b)
        worst, wsc = row_class_lib.stepped(s, o, params, b, K=4)
        row_class_lib.record("stepped_f64_vs_oracle", (p_max, name), worst, wsc)
        assert s.sched_error() == 0
        s.close()
        o.close()
        assert max(worst.values()) < 1e-10, (name, worst)
        row_class_lib.check_scalars(wsc, 1e-10)


@pytest.mark.parametrize("p_max", row_class_lib.CLASS_EDGES)
def test_stepped_iterates_float_storage(built, p_max):
    """Float storage (double arithmetic) on float-rounded inputs, four single outer iterations of both phases against the
    emulator in the same storage mode: every discrete decision identical, fields and continuous scalars within 1e-5;
    against the oracle (storage rounding, measured on the emulator: up to 8e-5 in the fields) within 3e-3.
    Measured against the emulator (first run): bit-identical at most edges; 6.4e-6 at most (S, p_max 128, phase 0), where
    one stored float rounds the other way (X / U 5e-8, one float ulp) and the slack rows carry it on."""
    batch = row_class_lib.edge_batch(p_max)
    for name, params, b in row_class_lib.phases(batch, f32=True):
        s, e = begun(params, b, np.float32), emuapi.EmuSolver(params, b, np.float32, True)
        worst, wsc = row_class_lib.stepped(s, e, params, b, K=4)
        row_class_lib.record("stepped_f32_vs_emulator", (p_max, name), worst, wsc)
        s.close()
        e.close()
        assert max(worst.values()) < 1e-5, (name, worst)
        row_class_lib.check_scalars(wsc, 1e-5)
        s, o = begun(params, b, np.float32), row_class_lib.Oracle(params, b)
        worst, wsc = row_class_lib.stepped(s, o, params, b, K=4)
        row_class_lib.record("stepped_f32_vs_oracle", (p_max, name), worst, wsc)
        s.close()
        o.close()
        assert max(worst.values()) < 3e-3, (name, worst)


def forms(p_max):
    """(name, environment, launch_info entries the launch must show) of every launch form of one class"""
    out = [("static", dict(DIRECT_DDP_SCHED="static"), dict(dynamic=0)),
           # a batch below the resident waves goes to the static launch unless it has helpers: fewer waves than tickets
           ("tickets", dict(DIRECT_DDP_HELP="0", DIRECT_DDP_SLOTS="8"), dict(dynamic=1, shared_search=0, shared_sweep=0)),
           ("help", dict(DIRECT_DDP_HELP="1"), dict(dynamic=1, shared_search=1)),
           ("help_few_waves", dict(DIRECT_DDP_HELP="1", DIRECT_DDP_SLOTS="8"), dict(dynamic=1, shared_search=1)),
           ("pair0", dict(DIRECT_DDP_HELP="1", DIRECT_DDP_PAIR="0"), dict(dynamic=1, pair_trials=0)),
           ("pair1", dict(DIRECT_DDP_HELP="1", DIRECT_DDP_PAIR="1"), dict(dynamic=1, pair_trials=1))]
    if helpers.row_class(p_max) <= 4:   # the sharing instantiations k_iterate_dyn<Real, 2 | 3 | 4, true>
        out += [("bshare%d" % m, dict(DIRECT_DDP_HELP="1", DIRECT_DDP_BSHARE=str(m)), dict(dynamic=1, shared_sweep=m))
                for m in (0, 1, 2)]
    return out


def assert_same(a, b, what):
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, f)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("p_max", CLASS_TOP)
def test_launch_forms_are_bitwise_equal(built, p_max, dt, monkeypatch):
    """24 problems with edge plane counts: a natural-exit plan (phase 1 iter_max = 30) and a fixed-20 phase-1 solve from the
    static launch's phase-0 result, every output bit-identical across the launch forms of the class, no scheduler error,
    and launch_info showing that each form was taken"""
    batch = row_class_lib.edge_batch(p_max, B=24, seed=3).astype(dt)
    p0, p1, pf = abi.phase0_params(), abi.phase1_params(iter_max=30), abi.phase1_params(iter_max=20, fixed_iters=1)
    keys = ("DIRECT_DDP_SCHED", "DIRECT_DDP_HELP", "DIRECT_DDP_SLOTS", "DIRECT_DDP_PAIR", "DIRECT_DDP_BSHARE")
    ref = b1 = None
    for name, env, want in forms(p_max):
        for k in keys:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = solver.DdpSolver(batch.batch, batch.n_seg_max, batch.p_max, dt)
        g0, g1 = s.plan(p0, p1, batch)
        assert s.sched_error() == 0, name
        if b1 is None:
            b1 = batch.phase1_inputs(g0)
        gf = s.solve(pf, b1)
        assert s.sched_error() == 0, name
        li = s.launch_info()
        s.close()
        for k, v in want.items():
            assert li[k] == v, (name, k, li)
        assert (gf.fwd_passes == 20).all(), name
        if ref is None:
            ref = (g0, g1, gf)
            assert g1.iter_used.max() > 1 and (g1.rtn >= 0).sum() >= 12, (g1.rtn, g1.iter_used)
        else:
            for a, b, what in zip(ref, (g0, g1, gf), ("phase0", "phase1", "fixed20")):
                assert_same(a, b, (name, what))


def mixed_batch(seed=0):
    """one problem per entry of CLASS_EDGES, on a 128-plane handle: every class is some problem's widest polytope"""
    pm = np.array(row_class_lib.CLASS_EDGES)
    base = problems.make_batch("corridor", len(pm), 9, seed=880 + seed)
    n_seg = 7 + np.arange(len(pm)) % 3
    b = helpers.with_edge_planes(helpers.ragged(base, n_seg), pm, seed=seed)
    assert b.p_max == 128 and sorted({helpers.row_class(int(p)) for p in b.n_planes.max(axis=1)}) == [2, 3, 4, 5, 6, 7, 8, 10, 12, 14]
    return b


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_mixed_classes_one_launch_and_class_launches_are_bitwise_equal(built, dt, monkeypatch):
    """One class-14 launch (slot_on skips the empty slots) and DIRECT_DDP_CLASSES=1 (the batch sorted into ten classes,
    Batch::idx, forked streams): natural-exit plan and fixed-20 solve bit-identical, with host inputs and with
    device-resident ones (the classes then come from k_classify)."""
    import torch
    from direct_amd import devmem
    dev = torch.device("cuda:0")
    batch = mixed_batch().astype(dt)
    B, N = batch.batch, batch.n_seg_max
    p0, p1, pf = abi.phase0_params(), abi.phase1_params(iter_max=30), abi.phase1_params(iter_max=20, fixed_iters=1)
    out, b1 = {}, None
    for mode in ("0", "1"):
        monkeypatch.setenv("DIRECT_DDP_CLASSES", mode)
        s = solver.DdpSolver(B, N, 128, dt)
        g0, g1 = s.plan(p0, p1, batch)
        if b1 is None:
            b1 = batch.phase1_inputs(g0)
        gf = s.solve(pf, b1)
        assert s.sched_error() == 0
        din, dfix = devmem.DeviceBatch(batch, dev), devmem.DeviceBatch(b1, dev)
        o0, o1, of = (devmem.DeviceResult(B, N, dt, dev) for _ in range(3))
        s.plan_device(p0, p1, din.cin, o0.cout, o1.cout)
        s.solve_device(pf, dfix.cin, of.cout)
        torch.cuda.synchronize()
        assert s.sched_error() == 0
        s.close()
        out[mode] = (g0, g1, gf)
        for what, o, g in (("phase0", o0, g0), ("phase1", o1, g1), ("fixed20", of, gf)):
            for k in ("rtn", "iter_used", "fwd_passes", "cost", "T", "bez", "poly"):
                assert np.array_equal(o[k].cpu().numpy(), np.asarray(getattr(g, k))), ("device inputs", mode, what, k)
    for a, b, what in zip(out["0"], out["1"], ("phase0", "phase1", "fixed20")):
        assert_same(a, b, what)
    assert (out["1"][2].fwd_passes == 20).all() and out["1"][1].iter_used.max() > 1


def test_mixed_classes_stepped_through_the_index_list(built, monkeypatch):
    """Under DIRECT_DDP_CLASSES=1 the stepwise interface runs the class launches too and reads every field back through
    the index list: three single outer iterations of both phases against the oracle (double storage, 1e-10).  Then S and
    Y of problems of six different classes are edited through set(), and one more iteration must match the oracle given
    the same edit."""
    monkeypatch.setenv("DIRECT_DDP_CLASSES", "1")
    batch = mixed_batch(seed=1)
    for name, params, b in row_class_lib.phases(batch):
        s, o = begun(params, b, np.float64), row_class_lib.Oracle(params, b)
        worst, wsc = row_class_lib.stepped(s, o, params, b, K=3)
        row_class_lib.record("mixed_classes_stepped_f64", name, worst, wsc)
        assert max(worst.values()) < 1e-10, (name, worst)
        row_class_lib.check_scalars(wsc, 1e-10)
        # scale the slacks (and duals) of one knot of problems in classes 2, 5, 7, 10, 12, 14 - each in its own class launch
        edit = [0, 5, 9, 13, 16, 18]
        assert [helpers.row_class(int(b.n_planes[i].max())) for i in edit] == [2, 5, 7, 10, 12, 14]
        fields = (abi.FIELD_S, abi.FIELD_Y) if params.infeas else (abi.FIELD_S,)
        for f in fields:
            got = s.get(f)
            for i in edit:
                k = 1 + i % (int(b.n_seg[i]) - 1)
                got[i, k] *= 1.25
                q = o.o.st[i]
                v = q.get(f)
                v[k] *= 1.25
                q.set(f, v)
            s.set(f, got)
        worst, wsc = row_class_lib.stepped(s, o, params, b, K=1)
        row_class_lib.record("mixed_classes_after_set_f64", name, worst, wsc)
        assert max(worst.values()) < 1e-10, (name, "after set", worst)
        row_class_lib.check_scalars(wsc, 1e-10)
        assert s.sched_error() == 0
        s.close()
        o.close()
