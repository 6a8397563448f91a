"""Pair rounds of the line search with both trials evaluated together in phases D and T (ddp_wave.h, Wave::run_round<2>).

A family of small feasible problems is solved with one step per sweep and with paired steps: free-space generator, B = 4,
N in {1, 2, 5, 12} (at N = 1 and N = 2 the first and the last knot of the joint path are the same knot / neighbours),
durations scaled by 0.5 and by 1.0 (short durations make step 0 fail often), phase-1 parameters after phase 0.  Every output
field of both phases must be equal byte for byte.

The family is only a test of the joint paths if its line searches really run them, so the test asserts that from the
single-step run (the accepted step of every line search through the stepwise interface) and from the oracle (a replay of
the rejected trials of oracle/direct_ref.c's forward pass, which tells at which knot each of them ended):

  odd     line searches accepted at an odd step: both trials of a pair alive to the last knot, the first one wins
  even    line searches accepted at an even nonzero step: the second trial of a pair wins
  switch  line searches accepted at an even nonzero step whose odd partner ended before the last knot: the sweep goes from
          the joint path to the single-alive path in its middle

Counts of the committed family (seed 2024 + N), line searches of phase 1 on which the oracle and the emulator's single-step
run agree, odd / even / switch - asserted below as FAMILY_COUNTS:

  N = 1   durations x 0.5: 24 / 15 / 0    x 1.0: 14 / 11 / 0     (one knot: nothing can end before the last)
  N = 2   durations x 0.5: 15 / 15 / 7    x 1.0: 18 /  9 / 0
  N = 5   durations x 0.5: 18 /  9 / 2    x 1.0: 14 /  8 / 0
  N = 12  durations x 0.5: 12 /  8 / 7    x 1.0: 10 /  7 / 2
  family: 125 / 82 / 18
"""
import numpy as np
import pytest

from direct_amd import abi, problems
from oracle import refapi
from tests.emu import emuapi

SEED = 2024
FAMILY = [(N, scale) for N in (1, 2, 5, 12) for scale in (0.5, 1.0)]
B = 4
FIELDS = ("rtn", "iter_used", "fwd_passes", "infeas_out", "cost", "costq", "opterr", "mu", "T", "poly", "bez")
# line searches of phase 1 over the whole family: accepted at an odd step, at an even nonzero step, joint -> single switches
FAMILY_COUNTS = dict(odd=125, even=82, switch=18)


def family_batch(N, scale, dtype=np.float64):
    b = problems.make_batch("free", B, N, seed=SEED + N)
    return b.with_init(None, T0=b.T0 * scale).astype(dtype)


def _first_failed_knot(pre, gains, params, batch, b, step):
    """Knot at which the trial of step size 2^-step leaves the fraction-to-boundary region (feasible mode, DDP:693-706),
    N when it reaches the end of the horizon: the forward roll of oracle/direct_ref.c from the oracle's own iterate and gains."""
    X, U, S, Cc, mu = pre
    KU, KUU, KS, KsM = gains
    N = U.shape[0]
    alpha, tau = 2.0 ** -step, max(0.99, 1.0 - mu)
    xn = X[0].copy()
    for i in range(N):
        P = int(batch.n_planes[b, i])
        nc = 6 * P + 55
        dx = xn - X[i]
        sn = S[i, :nc] + alpha * KS[i, :nc] + KsM[i, :nc] @ dx
        un = U[i] + alpha * KU[i] + KUU[i] @ dx
        cn = refapi.eval_c(params, xn, un, batch.planes[b, i, :P])[:nc]
        if (cn > (1 - tau) * Cc[i, :nc]).any() or (sn < (1 - tau) * S[i, :nc]).any():
            return i
        xn = refapi.eval_nextx(xn, un)
    return N


def oracle_events(params, batch):
    """Per trajectory: the accepted step of every line search of the oracle, and for the even nonzero ones the knot at which
    the odd partner ended."""
    out = []
    for b in range(batch.batch):
        st = refapi.Stepper(params, batch, b)
        steps = []
        for _ in range(params.iter_max):
            sc = st.scalars()
            feas = int(sc["infeas"]) == 0
            pre = (st.get(abi.FIELD_X), st.get(abi.FIELD_U), st.get(abi.FIELD_S), st.get(abi.FIELD_C), float(sc["mu"]))
            done = st.iterate(1)
            sc = st.scalars()
            step = -1 if int(sc["fp_failed"]) else int(sc["step"])
            partner_end = None
            if feas and step >= 2 and step % 2 == 0:
                gains = (st.get(abi.FIELD_KU), st.get(abi.FIELD_KUU), st.get(abi.FIELD_KS), st.get(106))
                partner_end = _first_failed_knot(pre, gains, params, batch, b, step - 1)
            steps.append((feas, step, partner_end))
            if done:
                break
        st.close()
        out.append(steps)
    return out


def emu_steps(params, batch):
    """Accepted step of every line search of the emulator's run, per trajectory (-1: the search failed)."""
    s = emuapi.EmuSolver(params, batch)
    hist = [[] for _ in range(batch.batch)]
    for _ in range(params.iter_max):
        before = s.scalars()
        if (before["done"] != 0).all():
            break
        s.iterate(1)
        after = s.scalars()
        for b in range(batch.batch):
            if before["done"][b] == 0:
                hist[b].append(-1 if after["fp_failed"][b] else int(after["step"][b]))
    s.close()
    return hist


def count_events(p1, b1, steps_emu):
    """odd / even / switch counts of one member of the family: a line search counts only where the emulator's single-step run
    accepted the very step the oracle accepted, in feasible mode."""
    n = dict(odd=0, even=0, switch=0)
    N = b1.n_seg_max
    for b, ora in enumerate(oracle_events(p1, b1)):
        for it, (feas, step, partner_end) in enumerate(ora):
            if not feas or it >= len(steps_emu[b]) or steps_emu[b][it] != step or step < 1:
                continue
            if step % 2:
                n["odd"] += 1
            else:
                n["even"] += 1
                if partner_end is not None and partner_end < N - 1:
                    n["switch"] += 1
    return n


def solve_family_member_emu(N, scale):
    batch = family_batch(N, scale)
    p0, p1 = abi.phase0_params(), abi.phase1_params()
    e0 = emuapi.solve_batch(p0, batch)
    b1 = batch.phase1_inputs(e0)
    return (p0, p1, batch, b1, e0, emuapi.solve_batch(p1, b1))


def test_joint_pair_rounds_are_bitwise_the_single_step_search_on_the_emulator(monkeypatch):
    """Emulator, DIRECT_EMU_PAIR=0 against =1, the whole family; the preconditions (odd / even / switch > 0) are counted on
    the single-step run and on the oracle and must be the committed FAMILY_COUNTS."""
    total = dict(odd=0, even=0, switch=0)
    for N, scale in FAMILY:
        monkeypatch.setenv("DIRECT_EMU_PAIR", "0")
        p0, p1, batch, b1, a0, a1 = solve_family_member_emu(N, scale)
        steps = emu_steps(p1, b1)
        monkeypatch.setenv("DIRECT_EMU_PAIR", "1")
        _, _, _, _, c0, c1 = solve_family_member_emu(N, scale)
        for ph, (a, c) in enumerate(((a0, c0), (a1, c1))):
            for f in FIELDS:
                x, y = np.ascontiguousarray(getattr(a, f)), np.ascontiguousarray(getattr(c, f))
                assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (N, scale, ph, f)
        n = count_events(p1, b1, steps)
        print("N = %d, durations x %.1f: %s" % (N, scale, n))
        for k in total:
            total[k] += n[k]
    print("family:", total)
    assert total["odd"] > 0 and total["even"] > 0 and total["switch"] > 0, total
    assert total == FAMILY_COUNTS, total


@pytest.mark.gpu
def test_joint_pair_rounds_are_bitwise_the_single_step_search_on_the_device(built, monkeypatch):
    """The same family through DdpSolver, float and double storage, DIRECT_DDP_PAIR=0 against =1 on fresh handles with the
    shared line search forced on (DIRECT_DDP_HELP=1: helper waves run joint rounds under the cancel poll): every output array
    bit for bit, no scheduler error."""
    from direct_amd import solver
    monkeypatch.setenv("DIRECT_DDP_HELP", "1")
    for dtype in (np.float32, np.float64):
        for N, scale in FAMILY:
            batch = family_batch(N, scale, dtype)
            res = {}
            for mode in ("0", "1"):
                monkeypatch.setenv("DIRECT_DDP_PAIR", mode)
                s = solver.DdpSolver(B, N, batch.p_max, dtype)
                res[mode] = s.plan(abi.phase0_params(), abi.phase1_params(), batch)
                assert s.sched_error() == 0
                s.close()
            for ph, (a, c) in enumerate(zip(res["0"], res["1"])):
                for f in FIELDS:
                    x, y = np.ascontiguousarray(getattr(a, f)), np.ascontiguousarray(getattr(c, f))
                    assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (dtype, N, scale, ph, f)
