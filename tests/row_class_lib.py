"""Stepped comparisons at the edges of the row-slot classes, shared by tests/test_emu_parity.py (lane-loop emulator) and
tests/test_gpu_row_classes.py (device).  TEST INFRASTRUCTURE.

The DDP kernels are instantiated for 2 .. 8, 10, 12 and 14 row slots of 64 per lane (direct_ddp.hip, rpl_class); a knot
has 6 P + 55 constraint rows.  CLASS_EDGES holds the lowest and the highest p_max of every class.  Batches are short and
ragged corridors whose knots sit at slot boundaries (helpers.with_edge_planes): row slots a knot leaves empty are skipped
(Wave::slot_on), row descriptors are reused across runs of equal plane counts (Wave::prefetch, pk_valid)."""
import json
import os

import numpy as np

from direct_amd import abi, problems
from oracle import refapi
from tests import helpers, soak_lib

CLASS_EDGES = (12, 13, 22, 23, 33, 34, 44, 45, 54, 55, 65, 66, 76, 77, 97, 98, 118, 119, 128)
CONTINUOUS = ("cost", "costq", "logcost", "err", "mu", "opterr", "stepsize")
DISCRETE = ("reg", "step", "fp_failed", "bp_failed", "rtn", "iter", "done", "filter_n", "infeas")


def edge_batch(p_max, B=6, seed=0):
    """B corridors of 7 .. 9 segments (ragged), plane counts at the slot boundaries up to p_max (knot 0: exactly p_max)"""
    base = problems.make_batch("corridor", B, 9, seed=600 + 7 * seed + p_max)
    n_seg = np.array([9, 7, 8][:B] + [int(x) for x in np.random.default_rng(seed + p_max).integers(7, 10, max(B - 3, 0))])
    b = helpers.with_edge_planes(helpers.ragged(base, n_seg), p_max, seed=1000 * seed + p_max)
    assert (b.n_planes[:, 0] == p_max).all() and helpers.row_class(int(b.n_planes.max())) == helpers.row_class(p_max)
    return b


def rounded(batch):
    """the float-rounded inputs, in double: what float storage sees"""
    return batch.astype(np.float32).astype(np.float64)


def phases(batch, f32=False):
    """[(name, params, inputs)] of both phases: phase 0 in infeasible mode, phase 1 in feasible mode from the ORACLE's
    phase-0 result (monomial hand-off, include/direct_ddp.h), so that every implementation starts both from the same
    inputs.  f32: every input float-rounded."""
    p0, p1 = abi.phase0_params(), abi.phase1_params()
    assert p0.infeas == 1 and p1.infeas == 0
    b0 = rounded(batch) if f32 else batch
    r0, _ = refapi.solve_batch(p0, b0)
    b1 = b0.phase1_inputs(r0)
    return [("phase0", p0, b0), ("phase1", p1, rounded(b1) if f32 else b1)]


class Oracle:
    """soak_lib.OracleStepper (frozen where the reference leaves its loop) with get() in the device's batch layout"""

    def __init__(self, params, batch):
        self.o = soak_lib.OracleStepper(params, batch)
        self.batch = batch

    def iterate(self, n):
        self.o.iterate(n)

    def scalars(self):
        return self.o.scalars()

    def backward(self):
        for s in self.o.st:
            s.backward()

    def get(self, field):
        b = self.batch
        shape = {abi.FIELD_X: (b.n_seg_max + 1, 9), abi.FIELD_U: (b.n_seg_max, 10), abi.FIELD_S: (b.n_seg_max, b.nc_max),
                 abi.FIELD_Y: (b.n_seg_max, b.nc_max), abi.FIELD_KU: (b.n_seg_max, 10), abi.FIELD_KUU: (b.n_seg_max, 10, 9),
                 abi.FIELD_KS: (b.n_seg_max, b.nc_max), abi.FIELD_KY: (b.n_seg_max, b.nc_max)}[field]
        out = np.zeros((b.batch,) + shape)
        for i, s in enumerate(self.o.st):
            v = s.get(field)
            out[(i,) + tuple(slice(0, n) for n in v.shape)] = v
        return out

    def close(self):
        self.o.close()


def field_dev(got, want, batch, field):
    """largest relative deviation over the problems (each relative to the problem's own largest entry), real knots only"""
    worst = 0.0
    for i in range(batch.batch):
        n = int(batch.n_seg[i]) + (1 if field == abi.FIELD_X else 0)
        worst = max(worst, helpers.rel(got[i, :n], want[i, :n]))
    return worst


def scalar_devs(sg, sr):
    """-> ({continuous scalar: largest relative deviation}, names of the discrete scalars that differ)"""
    d = {}
    for n in CONTINUOUS:
        a, b = np.asarray(sg[n], np.float64), np.asarray(sr[n], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-30))
        d[n] = float(r.max())
    flips = [n for n in DISCRETE if not np.array_equal(np.asarray(sg[n]).astype(np.int64), np.asarray(sr[n]).astype(np.int64))]
    return d, flips


def stepped(impl, ref, params, batch, K=4):
    """K single outer iterations of impl and ref side by side.  After each: every discrete decision identical (asserted)
    and the largest deviation of X / U / S / Y (Y in infeasible mode only) and of the continuous scalars.
    -> (dict field -> worst deviation over the K iterations, dict scalar -> worst deviation)"""
    fields = [("X", abi.FIELD_X), ("U", abi.FIELD_U), ("S", abi.FIELD_S)] + ([("Y", abi.FIELD_Y)] if params.infeas else [])
    worst = {n: 0.0 for n, _ in fields}
    wsc = {n: 0.0 for n in CONTINUOUS}
    for it in range(K):
        impl.iterate(1)
        ref.iterate(1)
        d, flips = scalar_devs(impl.scalars(), ref.scalars())
        assert not flips, (it, flips, {n: (impl.scalars()[n], ref.scalars()[n]) for n in flips})
        wsc = {n: max(wsc[n], d[n]) for n in CONTINUOUS}
        for n, f in fields:
            worst[n] = max(worst[n], field_dev(np.asarray(impl.get(f), np.float64), np.asarray(ref.get(f), np.float64), batch, f))
    return worst, wsc


def check_scalars(wsc, tol):
    """continuous scalars within tol; opterr (DDP:641, max |Qu| over the sweep: a gradient that cancels towards the
    optimum, read only by the barrier update whose outcome mu is held to tol) within 100 tol"""
    for n, v in wsc.items():
        assert v < (100 * tol if n == "opterr" else tol), (n, v, wsc)


def record(test, key, worst, wsc=None):
    """appends the measured worst deviations to the JSON-lines file DIRECT_ROW_CLASS_REPORT names (if set): the figures
    the bounds of the row-class tests rest on"""
    path = os.environ.get("DIRECT_ROW_CLASS_REPORT")
    if path:
        rec = dict(test=test, key=key, fields={k: float(v) for k, v in worst.items()})
        if wsc is not None:
            rec["scalars"] = {k: float(v) for k, v in wsc.items()}
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
