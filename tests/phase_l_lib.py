"""Batches for phase L of the DDP knots (Wave::prefetch / Wave::commit and the knot addresses of Wave::set_sweep_ptrs,
direct_amd/csrc/ddp_wave.h), shared by tests/test_emu_phase_l.py (lane-loop emulator) and tests/test_gpu_phase_l.py
(device).  TEST INFRASTRUCTURE.

Phase L is the head of every knot: it commits the prefetched words of the knot to LDS and issues the loads of the next one
from clamped per-lane indices.  What can go wrong there depends on the horizon and on the plane counts, not on the size of
the batch, so every batch here has three trajectories:

  * N = 1, 2, 3 and 7 segments: the `k + 1 < N` / `k + 2 < N` clamps of the prefetch and of the plane count that runs two
    knots ahead (forward), `k > 0` / `k > 1` (backward);
  * trajectories 0 and 2 change their plane count P from knot to knot, so the row descriptors (and whatever else is kept
    per run of equal P) are rebuilt in the middle of both sweeps.  The counts sit on the boundaries of the per-lane words:
    P = 1 (4 P - 1 = 3: nearly every lane of the plane words clamped), 10 and 11 (6 P rows across 64: the second
    position-row slot appears), 12 (top of the two-slot class), 16 and 17 (4 P = 64 exactly, then the second plane word),
    22 and 33 (tops of the three- and four-slot classes), 40 (a five-slot class: no wide gather, per-knot slot skipping);
  * trajectory 1 keeps P = 6 throughout: nothing is ever rebuilt after knot 0, the path of a free-space corridor.

CLASSES gives the batches per kernel class: the handle's p_max is the width of the planes array, so "two" runs the two-slot
kernels (p_max 12), "three" and "four" the next ones (22, 33) and "wide" a five-slot kernel (40).  Durations are scaled
by 0.5 / 1.0 / 0.7 (trajectories 0 / 1 / 2; as in tests/test_pair_round_joint.py): trajectory 0 mostly stays infeasible
through phase 0 and runs phase 1 in infeasible mode, the other two run it in feasible mode, where step 0 of the line
searches fails often, the searches go on to paired steps, and a pair loses a partner in the middle of a sweep (all of it
asserted from the oracle, test_emu_phase_l.py)."""
import hashlib

import numpy as np

from direct_amd import abi, problems

SEED = 7300
B = 3
N_CASES = (1, 2, 3, 7)
ITERS = 3
DURATION_SCALE = (0.5, 1.0, 0.7)   # per trajectory
# class -> (p_max of the handle, plane counts per knot of trajectories 0, 1, 2; a batch of N segments takes the first N)
CLASSES = {
    "two": (12, ((1, 10, 11, 12, 1, 11, 10), (6,) * 7, (12, 12, 10, 1, 1, 11, 12))),
    "three": (22, ((16, 17, 22, 10, 11, 17, 16), (6,) * 7, (22, 1, 17, 17, 12, 16, 22))),
    "four": (33, ((33, 22, 17, 16, 33, 1, 12), (6,) * 7, (23, 33, 33, 11, 10, 17, 1))),
    "wide": (40, ((40, 33, 1, 17, 40, 10, 22), (6,) * 7, (16, 40, 40, 11, 12, 33, 1))),
}
OUT_FIELDS = tuple(n for n, _ in abi.BatchOut._fields_[1:])   # every array of direct_ddp_batch_out_t


def with_plane_counts(batch, counts, width, seed):
    """The corridors of `batch` with exactly counts[b][k] planes at knot k of problem b, in a planes array `width` wide.
    A count above the polytope's own is padded with half-spaces through points 0.8 .. 3 m outside both seeds of the segment
    (valid, mostly inactive: tests/helpers.py with_extra_planes); a count below it keeps the polytope's first planes."""
    rng = np.random.default_rng(seed)
    nb, nm, p0 = batch.planes.shape[:3]
    planes = np.zeros((nb, nm, max(width, p0), 4))
    planes[:, :, :p0] = batch.planes
    n_planes = batch.n_planes.copy()
    for b in range(nb):
        for k in range(int(batch.n_seg[b])):
            target = int(counts[b][k])
            a = batch.x0[b, :3] if k == 0 else batch.seeds[b, k]
            c = batch.xd[b, :3] if k == batch.n_seg[b] - 1 else batch.seeds[b, k + 1]
            j = min(int(n_planes[b, k]), target)
            planes[b, k, j:] = 0.0
            while j < target:
                n = rng.normal(size=3)
                n /= np.linalg.norm(n)
                off = max(float(n @ a), float(n @ c)) + float(rng.uniform(0.8, 3.0))   # both seeds strictly inside
                planes[b, k, j] = np.r_[n, -off]
                j += 1
            n_planes[b, k] = target
    planes = np.ascontiguousarray(planes[:, :, :width])
    return abi.HostBatch(batch.n_seg, batch.x0, batch.xd, batch.T0, n_planes, planes, seeds=batch.seeds, dtype=batch.dtype)


def make(cls, N, dtype=np.float64):
    """the batch of class `cls` with N segments (seed SEED + N for the corridors, SEED + 100 + N for the padding planes)"""
    width, counts = CLASSES[cls]
    base = problems.make_batch("corridor", B, N, seed=SEED + N)
    b = with_plane_counts(base, [c[:N] for c in counts], width, SEED + 100 + N)
    assert b.p_max == width and (b.n_planes[1] == 6).all() and int(b.n_planes.max()) <= width
    return b.with_init(None, T0=b.T0 * np.array(DURATION_SCALE)[:, None]).astype(dtype)


def fixed(params_fn):
    """ITERS fixed outer iterations of a phase"""
    return params_fn(iter_max=ITERS, fixed_iters=1)


def digest(batch):
    """of every input array: the recorded device results belong to exactly these inputs"""
    h = hashlib.sha256()
    for a in (batch.n_seg, batch.x0, batch.xd, batch.T0, batch.n_planes, batch.planes, batch.seeds):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def device_results(cls, N, dtype):
    """-> ({name: HostResult}, digest of the inputs, launch_info of the last solve) of one handle on the batch: phase 0 with its natural exit ("p0"), ITERS fixed
    iterations of phase 0 ("p0fix": infeasible mode, the dual rows) and ITERS fixed iterations of phase 1 from the natural
    phase-0 result ("p1fix": feasible and infeasible trajectories side by side); the launch form is the caller's environment"""
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
