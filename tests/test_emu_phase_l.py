"""Phase L of the DDP knots on the lane-loop emulator of the kernels' own source (tests/phase_l_lib.py): horizons of
1, 2, 3 and 7 segments, plane counts that change from knot to knot on every boundary of the per-lane index and predicate
words, next to a trajectory of constant P = 6, in the two-, three-, four- and a five-slot kernel class.

Three single outer iterations of both phases side by side with the oracle: every discrete decision identical after each,
X / U / S / Y (Y in infeasible mode) and the continuous scalars within 1e-10 per problem in double storage (the bound of
tests/test_emu_parity.py), and within 3e-3 in float storage on float-rounded inputs (the bound tests/test_gpu_row_classes.py
holds the same comparison to: what is compared there is storage rounding, a float per slack / dual row and iteration).

The batches are only a test of phase 1's two modes and of the pair round's single-alive path if they really get there;
test_batches_reach_what_they_are_for asserts it, from the oracle: seeds phase_l_lib.SEED + N (corridors) and
SEED + 100 + N (padding planes), durations scaled by phase_l_lib.DURATION_SCALE."""
import numpy as np
import pytest

from direct_amd import abi
from oracle import refapi
from tests import phase_l_lib, row_class_lib
from tests import test_pair_round_joint as pair_events
from tests.emu import emuapi

CASES = [(cls, N) for cls in phase_l_lib.CLASSES for N in phase_l_lib.N_CASES]


@pytest.mark.parametrize("cls,N", CASES)
def test_stepped_iterates_double_storage(cls, N):
    batch = phase_l_lib.make(cls, N)
    for name, params, b in row_class_lib.phases(batch):
        e, o = emuapi.EmuSolver(params, b), row_class_lib.Oracle(params, b)
        worst, wsc = row_class_lib.stepped(e, o, params, b, K=phase_l_lib.ITERS)
        e.close()
        o.close()
        print(cls, N, name, worst, wsc)
        assert max(worst.values()) < 1e-10, (name, worst)
        row_class_lib.check_scalars(wsc, 1e-10)


@pytest.mark.parametrize("cls,N", CASES)
def test_stepped_iterates_float_storage(cls, N):
    batch = phase_l_lib.make(cls, N)
    for name, params, b in row_class_lib.phases(batch, f32=True):
        e, o = emuapi.EmuSolver(params, b, np.float32, True), row_class_lib.Oracle(params, b)
        worst, wsc = row_class_lib.stepped(e, o, params, b, K=phase_l_lib.ITERS)
        e.close()
        o.close()
        print(cls, N, name, worst, wsc)
        assert max(worst.values()) < 3e-3, (name, worst)


def test_batches_reach_what_they_are_for():
    """Over the batches of the two-slot class (the class of the pair rounds' wide gather) and every horizon: phase 0 of the
    oracle leaves at least one trajectory feasible and at least one infeasible for phase 1, and within the three phase-1
    iterations a line search is accepted at an even nonzero step whose odd partner ended before the last knot - the
    pair round goes on with one trial alive from the middle of its sweep (counted as in tests/test_pair_round_joint.py)."""
    feasible = infeasible = 0
    events = dict(odd=0, even=0, switch=0)
    p1 = phase_l_lib.fixed(abi.phase1_params)
    for cls, N in CASES:
        batch = phase_l_lib.make(cls, N)
        r0, _ = refapi.solve_batch(abi.phase0_params(), batch)
        feasible += int((np.asarray(r0.infeas_out) == 0).sum())
        infeasible += int((np.asarray(r0.infeas_out) != 0).sum())
        if cls == "two":
            b1 = batch.phase1_inputs(r0)
            n = pair_events.count_events(p1, b1, pair_events.emu_steps(p1, b1))
            print(cls, N, "infeas_out", r0.infeas_out, n)
            for k in events:
                events[k] += n[k]
    print("feasible", feasible, "infeasible", infeasible, events)
    assert feasible > 0 and infeasible > 0, (feasible, infeasible)
    assert events["switch"] > 0 and events["odd"] > 0, events
