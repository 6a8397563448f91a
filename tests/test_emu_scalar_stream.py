"""Lane predicates and mode dispatch of the DDP knots on the lane-loop emulator of the kernels' own source
(tests/scalar_stream_lib.py): horizons of 1, 2, 3 and 7 segments, plane counts 1 / 10 / 11 / 21 / 22 / 32 / 33 that change from
knot to knot next to a trajectory of constant P = 6, in the two-, three-, four- and a five-slot kernel class.  The emulator
takes the same source as the device, so a store that a lane sends to a dump slot lands in its LDS struct as well.

Three single outer iterations of both phases side by side with the oracle: every discrete decision identical after each,
X / U / S / Y (Y in infeasible mode) and the continuous scalars within 1e-10 per problem in double storage and within 3e-3 in
float storage on float-rounded inputs - the bounds of tests/test_emu_phase_l.py, which holds the same comparison.

test_batches_reach_what_they_are_for asserts from the oracle that the batches are a test of both modes, of both sides of
every slot boundary in either mode, and of the pair round's single-alive path."""
import numpy as np
import pytest

from direct_amd import abi
from oracle import refapi
from tests import row_class_lib
from tests import scalar_stream_lib as lib
from tests import test_pair_round_joint as pair_events
from tests.emu import emuapi

CASES = [(cls, N) for cls in lib.CLASSES for N in lib.N_CASES]
BOUNDARY_COUNTS = {1, 10, 11, 21, 22, 32, 33}


@pytest.mark.parametrize("cls,N", CASES)
def test_stepped_iterates_double_storage(cls, N):
    batch = lib.make(cls, N)
    for name, params, b in row_class_lib.phases(batch):
        e, o = emuapi.EmuSolver(params, b), row_class_lib.Oracle(params, b)
        worst, wsc = row_class_lib.stepped(e, o, params, b, K=lib.ITERS)
        e.close()
        o.close()
        print(cls, N, name, worst, wsc)
        assert max(worst.values()) < 1e-10, (name, worst)
        row_class_lib.check_scalars(wsc, 1e-10)


@pytest.mark.parametrize("cls,N", CASES)
def test_stepped_iterates_float_storage(cls, N):
    batch = lib.make(cls, N)
    for name, params, b in row_class_lib.phases(batch, f32=True):
        e, o = emuapi.EmuSolver(params, b, np.float32, True), row_class_lib.Oracle(params, b)
        worst, wsc = row_class_lib.stepped(e, o, params, b, K=lib.ITERS)
        e.close()
        o.close()
        print(cls, N, name, worst, wsc)
        assert max(worst.values()) < 3e-3, (name, worst)


def test_batches_reach_what_they_are_for():
    """Over every class and horizon, from the oracle's phase 0: some batch hands phase 1 a feasible and an infeasible
    trajectory TOGETHER (one launch, both bodies of the mode dispatch); the knots of the trajectories that run phase 1 in
    feasible mode, and those of the ones that run it in infeasible mode, each see every plane count on either side of the
    slot boundaries (1 | 10, 11 | 21, 22 | 32, 33); and, in the two-slot class (the class of the pair rounds' wide gather),
    a line search of the three phase-1 iterations is accepted at an even nonzero step whose odd partner ended before the
    last knot - the pair round goes on with one trial alive from the middle of its sweep (counted as in
    tests/test_pair_round_joint.py)."""
    side_by_side = 0
    seen = {0: set(), 1: set()}   # mode of phase 1 -> plane counts of its trajectories' knots
    events = dict(odd=0, even=0, switch=0)
    p1 = lib.fixed(abi.phase1_params)
    for cls, N in CASES:
        batch = lib.make(cls, N)
        r0, _ = refapi.solve_batch(abi.phase0_params(), batch)
        mode = (np.asarray(r0.infeas_out) != 0).astype(int)
        side_by_side += int(mode.min() == 0 and mode.max() == 1)
        for b in range(lib.B):
            seen[int(mode[b])].update(int(p) for p in batch.n_planes[b, :N])
        if cls == "two":
            b1 = batch.phase1_inputs(r0)
            n = pair_events.count_events(p1, b1, pair_events.emu_steps(p1, b1))
            print(cls, N, "infeas_out", r0.infeas_out, n)
            for k in events:
                events[k] += n[k]
    print("side by side", side_by_side, "plane counts per mode", seen, events)
    assert side_by_side > 0
    assert BOUNDARY_COUNTS <= seen[0] and BOUNDARY_COUNTS <= seen[1], seen
    assert events["switch"] > 0 and events["odd"] > 0, events
