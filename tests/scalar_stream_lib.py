"""Batches for the lane predicates and the mode dispatch of the DDP knots (Wave::bwd_knot, Wave::run_round, Wave::commit and
the row phases, direct_amd/csrc/ddp_wave.h), shared by tests/test_emu_scalar_stream.py (lane-loop emulator) and
tests/test_gpu_scalar_stream.py (device).  TEST INFRASTRUCTURE.

What a lane predicate or a per-slot mode test can get wrong depends on where the row count 6 P + 55 of a knot falls within
the 64 lanes of a row slot, on the mode of the sweep and on the horizon - not on the size of the batch:

  * plane counts P = 1, 10, 11, 21, 22, 32, 33 (tests/phase_l_lib.py covers 12, 16, 17 and 40): 6 P + 55 = 61 leaves three
    lanes of the first slot idle, 115 / 121 and 181 / 187 and 247 / 253 sit 13 and 7 (11 and 5, 9 and 3) lanes below the
    top of the second, third and fourth slot: the last rows of a slot's lanes are live in one knot and idle in the next.
    Trajectories 0 and 2 change P from knot to knot, so the row descriptors are rebuilt in the middle of both sweeps;
  * trajectory 1 keeps P = 6 throughout, the path of a free-space corridor;
  * N = 1, 2, 3 and 7 segments: prologue only, one trip, and the exits of the knot loops;
  * durations scaled per trajectory (DURATION_SCALE): trajectory 0 mostly stays infeasible through phase 0 and runs phase 1
    in infeasible mode NEXT TO the other two in feasible mode - one launch, both bodies of every mode dispatch; in feasible
    mode step 0 of the line searches fails often, the searches go on to paired steps and a pair loses a partner in the
    middle of a sweep.  All of it is asserted from the oracle (tests/test_emu_scalar_stream.py).

CLASSES gives the batches per kernel class (p_max of the handle: 12, 22, 33 run the two-, three- and four-slot kernels, 40 a
five-slot one-wave kernel)."""
import numpy as np

from direct_amd import abi, problems
from tests import phase_l_lib

SEED = 7400
B = 3
N_CASES = (1, 2, 3, 7)
ITERS = 3
DURATION_SCALE = (0.5, 1.0, 0.7)   # per trajectory
# class -> (p_max of the handle, plane counts per knot of trajectories 0, 1, 2; a batch of N segments takes the first N)
CLASSES = {
    "two": (12, ((10, 11, 1, 11, 10, 1, 11), (6,) * 7, (11, 1, 10, 10, 11, 1, 10))),
    "three": (22, ((21, 22, 10, 11, 22, 21, 1), (6,) * 7, (22, 21, 21, 1, 11, 10, 22))),
    "four": (33, ((32, 33, 21, 22, 33, 10, 32), (6,) * 7, (33, 32, 32, 11, 1, 22, 33))),
    "five": (40, ((33, 32, 1, 22, 21, 11, 10), (6,) * 7, (10, 33, 32, 21, 33, 1, 22))),
}
OUT_FIELDS = phase_l_lib.OUT_FIELDS   # every array of direct_ddp_batch_out_t
digest = phase_l_lib.digest


def make(cls, N, dtype=np.float64):
    """the batch of class `cls` with N segments (seed SEED + N for the corridors, SEED + 100 + N for the padding planes)"""
    width, counts = CLASSES[cls]
    base = problems.make_batch("corridor", B, N, seed=SEED + N)
    b = phase_l_lib.with_plane_counts(base, [c[:N] for c in counts], width, SEED + 100 + N)
    assert b.p_max == width and (b.n_planes[1] == 6).all() and int(b.n_planes.max()) <= width
    return b.with_init(None, T0=b.T0 * np.array(DURATION_SCALE)[:, None]).astype(dtype)


def fixed(params_fn):
    """ITERS fixed outer iterations of a phase"""
    return params_fn(iter_max=ITERS, fixed_iters=1)


def device_results(cls, N, dtype):
    """-> ({name: HostResult}, digest of the inputs, launch_info of the last solve) of one handle on the batch: phase 0 with
    its natural exit ("p0"), ITERS fixed iterations of phase 0 ("p0fix": infeasible mode, the dual rows) and ITERS fixed
    iterations of phase 1 from the natural phase-0 result ("p1fix": feasible and infeasible trajectories side by side);
    the launch form is the caller's environment"""
    from direct_amd import solver
    batch = make(cls, N, dtype)
    s = solver.DdpSolver(B, N, batch.p_max, dtype)
    out = {}
    out["p0"] = s.solve(abi.phase0_params(), batch)
    assert s.sched_error() == 0
    out["p0fix"] = s.solve(fixed(abi.phase0_params), batch)
    assert s.sched_error() == 0
    out["p1fix"] = s.solve(fixed(abi.phase1_params), batch.phase1_inputs(out["p0"]))
    assert s.sched_error() == 0
    info = s.launch_info()
    s.close()
    return out, digest(batch), info


def key(cls, N, dtype, solve, field):
    return "%s_n%d_%s_%s_%s" % (cls, N, np.dtype(dtype).name, solve, field)
