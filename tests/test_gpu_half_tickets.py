"""Half-trip tickets of the ticket scheduler (DIRECT_DDP_HALF=1; direct_amd/csrc/sched_ticket.h): the
backward sweep with its retries and the line search with the exit rules of one outer iteration are drawn as two tickets
and may run on different waves.  Scheduling only - every case compares EVERY field of the output struct byte for byte with
the whole-trip launch (and the static one), and asks for sched_error() == 0 and a launch_info that shows the form taken."""
import numpy as np
import pytest

from direct_amd import abi, problems, solver
from tests import helpers, stuck_lib

pytestmark = pytest.mark.gpu

FIELDS = ("rtn", "iter_used", "fwd_passes", "infeas_out", "line_failed_out", "cost", "costq", "jerk_cost", "terminal_norm2",
          "opterr", "mu", "bez", "poly", "T")
KEYS = ("DIRECT_DDP_SCHED", "DIRECT_DDP_HELP", "DIRECT_DDP_SLOTS", "DIRECT_DDP_PAIR", "DIRECT_DDP_BSHARE", "DIRECT_DDP_HALF",
        "DIRECT_DDP_CHUNK", "DIRECT_DDP_TAIL")


def set_env(monkeypatch, env):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def assert_same(a, b, what):
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, f)


def make(batch, dt, flags=None):
    if flags is None:
        return solver.DdpSolver(batch.batch, batch.n_seg_max, batch.p_max, dt)
    return solver.DdpSolver(batch.batch, batch.n_seg_max, batch.p_max, dt, flags=flags)


def natural_and_fixed(monkeypatch, batch, dt, forms, n_fixed=6, b1=None):
    """phase 0 and phase 1 (from the FIRST form's phase-0 result) with their natural exits, then n_fixed fixed phase-1
    iterations, per form (name, environment, launch_info entries); returns {name: (phase 0, phase 1, fixed)}"""
    p1, pf = abi.phase1_params(iter_max=30), abi.phase1_params(iter_max=n_fixed, fixed_iters=1)
    out = {}
    for name, env, want in forms:
        set_env(monkeypatch, env)
        s = make(batch, dt)
        g0 = s.solve(abi.phase0_params(), batch)
        assert s.sched_error() == 0, name
        li0 = s.launch_info()
        if b1 is None:
            b1 = batch.phase1_inputs(g0)
        g1 = s.solve(p1, b1)
        assert s.sched_error() == 0, name
        li1 = s.launch_info()
        gf = s.solve(pf, b1)
        assert s.sched_error() == 0, name
        li = s.launch_info()
        s.close()
        for k, v in want.items():
            assert li0[k] == v and li1[k] == v and li[k] == v, (name, k, li0, li1, li)
        assert (gf.fwd_passes == n_fixed).all(), (name, gf.fwd_passes)
        out[name] = (g0, g1, gf)
    first = forms[0][0]
    assert out[first][1].fwd_passes.max() > 2, out[first][1].fwd_passes   # the natural exits are not all immediate
    for name, _, _ in forms[1:]:
        for i, what in enumerate(("phase0", "phase1", "fixed")):
            assert_same(out[first][i], out[name][i], (name, what))
    return out


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,N", [("free", 8), ("corridor", 12)])
def test_few_waves_late_starts_half_whole_and_static_agree(built, monkeypatch, kind, N, dt):
    """B = 7 on three persistent waves: trajectories start late and every unit waits for its predecessor on another wave"""
    batch = problems.make_batch(kind, 7, N, seed=311).astype(dt)
    forms = [("whole", dict(DIRECT_DDP_SLOTS="3", DIRECT_DDP_HALF="0"), dict(dynamic=1, half_tickets=0, shared_search=0)),
             ("half", dict(DIRECT_DDP_SLOTS="3", DIRECT_DDP_HALF="1"), dict(dynamic=1, half_tickets=1, shared_search=0)),
             ("half_chunk2", dict(DIRECT_DDP_SLOTS="3", DIRECT_DDP_HALF="1", DIRECT_DDP_CHUNK="2"), dict(dynamic=1, half_tickets=1)),
             ("static", dict(DIRECT_DDP_SCHED="static"), dict(dynamic=0, half_tickets=0))]
    natural_and_fixed(monkeypatch, batch, dt, forms)


@pytest.mark.parametrize("pair", ["0", "1"])
@pytest.mark.parametrize("kind,N", [("free", 12), ("corridor", 8)])
def test_helpers_with_and_without_pairs(built, monkeypatch, kind, N, pair):
    """B = 40 on twelve waves with the shared line search: waiters for either half help the open search"""
    batch = problems.make_batch(kind, 40, N, seed=312).astype(np.float32)
    env = dict(DIRECT_DDP_SLOTS="12", DIRECT_DDP_HELP="1", DIRECT_DDP_PAIR=pair)
    forms = [("whole", dict(env, DIRECT_DDP_HALF="0"), dict(dynamic=1, half_tickets=0, shared_search=1, pair_trials=int(pair))),
             ("half", dict(env, DIRECT_DDP_HALF="1"), dict(dynamic=1, half_tickets=1, shared_search=1, pair_trials=int(pair))),
             ("half_no_tail", dict(env, DIRECT_DDP_HALF="1", DIRECT_DDP_TAIL="0"), dict(dynamic=1, half_tickets=1))]
    natural_and_fixed(monkeypatch, batch, np.float32, forms)


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_shared_backward_sweeps(built, monkeypatch, mode):
    """B = 2, N = 100 on the sharing instantiation: a wave that waits for a line-search unit while the backward half runs
    joins the shared sweep (DIRECT_DDP_BSHARE=1), the forced split (2) and the owner-only sweep (0)"""
    batch = problems.make_batch("free", 2, 100, seed=313).astype(np.float32)
    env = dict(DIRECT_DDP_HELP="1", DIRECT_DDP_BSHARE=mode)
    forms = [("whole", dict(env, DIRECT_DDP_HALF="0"), dict(dynamic=1, half_tickets=0, shared_sweep=int(mode))),
             ("half", dict(env, DIRECT_DDP_HALF="1"), dict(dynamic=1, half_tickets=1, shared_sweep=int(mode)))]
    natural_and_fixed(monkeypatch, batch, np.float32, forms, n_fixed=4)


@pytest.mark.parametrize("dt,N", [(np.float64, 8), (np.float32, 12)], ids=["f64", "f32"])
def test_a_parked_trajectory_among_five_that_are_not(built, monkeypatch, dt, N):
    """The forced rtn = -4 scenario of tests/stuck_lib.py ("phase0_late": fixed iterations, K = 9) on trajectory 0 only: its
    backward half parks it in iteration K + 1 (kRtnStuckPending, finished by k_stuck), every later unit of it returns at
    once, the other five run their three iterations"""
    name, p, kind, K, y_inject, _ = stuck_lib.scenarios()[1]
    assert name == "phase0_late" and p.fixed_iters == 1
    batch = problems.make_batch(kind, 6, N, seed=77)
    sc = stuck_lib.Scenario(p, batch, K, y_inject)
    row, knot = sc.rows[0], sc.knot
    sc.close()
    batch = batch.astype(dt)
    res = {}
    for half in ("0", "1"):
        set_env(monkeypatch, dict(DIRECT_DDP_SLOTS="2", DIRECT_DDP_HALF=half))
        s = make(batch, dt)
        s.begin(p, batch)
        s.iterate(K)
        Y = s.get(abi.FIELD_Y)
        Y[0, knot, row] = y_inject
        s.set(abi.FIELD_Y, Y)
        s.iterate(3)
        li = s.launch_info()
        sca = s.scalars()
        fields = [s.get(f) for f in (abi.FIELD_X, abi.FIELD_U, abi.FIELD_S, abi.FIELD_Y)]
        res[half] = (s.finish(), {k: np.array(v) for k, v in sca.items()}, fields)
        assert s.sched_error() == 0
        s.close()
        assert li["dynamic"] == 1 and li["half_tickets"] == int(half), li
    w, h = res["0"], res["1"]
    assert w[0].rtn[0] == -4 and w[0].iter_used[0] == K and w[0].fwd_passes[0] == K + 1, (w[0].rtn, w[0].iter_used, w[0].fwd_passes)
    assert (w[0].rtn[1:] != -4).all() and (w[0].fwd_passes[1:] == K + 3).all(), (w[0].rtn, w[0].fwd_passes)
    assert_same(w[0], h[0], "stuck")
    for k in w[1]:
        assert w[1][k].tobytes() == h[1][k].tobytes(), k
    for a, b in zip(w[2], h[2]):
        assert a.tobytes() == b.tobytes()


def test_natural_exits_at_differing_iterations(built, monkeypatch):
    """B = 16 with 3 .. 12 segments, phase 0 -> phase 1 with natural exits: the units behind a finished trajectory are
    skipped and leave fwd_passes, iter_used and rtn alone"""
    base = problems.make_batch("corridor", 16, 12, seed=315)
    batch = helpers.ragged(base, 3 + np.arange(16) % 10).astype(np.float32)
    p0, p1 = abi.phase0_params(), abi.phase1_params(iter_max=30)
    res = {}
    for name, env in (("whole", dict(DIRECT_DDP_SLOTS="5", DIRECT_DDP_HALF="0")), ("half", dict(DIRECT_DDP_SLOTS="5", DIRECT_DDP_HALF="1")),
                      ("static", dict(DIRECT_DDP_SCHED="static"))):
        set_env(monkeypatch, env)
        s = make(batch, np.float32)
        res[name] = s.plan(p0, p1, batch)
        assert s.sched_error() == 0, name
        li = s.launch_info()
        s.close()
        assert li["dynamic"] == (name != "static") and li["half_tickets"] == (name == "half"), (name, li)
    for ph in (0, 1):
        w = res["whole"][ph]
        assert len(set(w.iter_used.tolist())) >= 3, w.iter_used   # the exits really differ
        for f in ("fwd_passes", "iter_used", "rtn"):
            assert np.array_equal(getattr(w, f), getattr(res["half"][ph], f)), (ph, f)
        assert_same(w, res["half"][ph], ("half", ph))
        assert_same(w, res["static"][ph], ("static", ph))


def test_stepwise_launches_of_one_iteration(built, monkeypatch):
    """direct_ddp_iterate(h, 1) x 4 == one launch of 4, whole and half tickets: a launch of one iteration is two units"""
    batch = problems.make_batch("corridor", 7, 8, seed=316).astype(np.float32)
    p = abi.phase0_params(fixed_iters=1)
    res = {}
    for half in ("0", "1"):
        for steps in ((1, 1, 1, 1), (4,)):
            set_env(monkeypatch, dict(DIRECT_DDP_SLOTS="3", DIRECT_DDP_HALF=half))
            s = make(batch, np.float32)
            s.begin(p, batch)
            for n in steps:
                s.iterate(n)
                li = s.launch_info()
                assert li["dynamic"] == 1 and li["half_tickets"] == int(half), li
            res[half, steps] = s.finish()
            assert s.sched_error() == 0
            s.close()
    ref = res["0", (4,)]
    assert (ref.fwd_passes == 4).all(), ref.fwd_passes
    for k, r in res.items():
        assert_same(ref, r, k)


def test_two_yielding_handles_alternate(built, monkeypatch):
    """Two DIRECT_FLAG_YIELD handles created once and kept, B = 33, four launches alternating between them on their own
    streams with half tickets: each bit-identical to a serial whole-ticket launch of an ordinary handle (the yield
    rule counts trajectories, not units)"""
    import torch
    from direct_amd import devmem
    dev = torch.device("cuda:0")
    dt, nb, N = np.float32, 33, 12
    batch = problems.make_batch("corridor", nb, N, seed=317).astype(dt)
    set_env(monkeypatch, dict(DIRECT_DDP_HALF="0"))
    one = make(batch, dt)
    g0 = one.solve(abi.phase0_params(), batch)
    b1 = batch.phase1_inputs(g0)
    din = devmem.DeviceBatch(b1, dev)
    ref = devmem.DeviceResult(nb, N, dt, dev)
    set_env(monkeypatch, dict(DIRECT_DDP_HALF="1"))
    hs = [make(batch, dt, flags=abi.FLAG_YIELD) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    for h, st in zip(hs, streams):
        h.set_stream(st.cuda_stream)
    outs = [devmem.DeviceResult(nb, N, dt, dev) for _ in range(4)]
    for p in (abi.phase1_params(iter_max=6, fixed_iters=1), abi.phase1_params(iter_max=30)):
        one.solve_device(p, din.cin, ref.cout)
        torch.cuda.synchronize()
        assert one.launch_info()["half_tickets"] == 0
        for i in range(4):
            hs[i % 2].solve_device(p, din.cin, outs[i].cout)
        torch.cuda.synchronize()
        assert one.sched_error() == 0 and all(h.sched_error() == 0 for h in hs)
        for h in hs:
            li = h.launch_info()
            assert li["dynamic"] == 1 and li["half_tickets"] == 1, li
        for i in range(4):
            for k in ref.t:
                assert torch.equal(outs[i].t[k], ref.t[k]), (i, k, p.fixed_iters)
    for h in hs + [one]:
        h.close()
