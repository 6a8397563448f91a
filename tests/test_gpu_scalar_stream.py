"""Lane predicates and mode dispatch of the DDP knots on the device (tests/scalar_stream_lib.py): horizons of 1, 2, 3 and 7
segments; plane counts 1 / 10 / 11 / 21 / 22 / 32 / 33 that change from knot to knot, so that the last live row moves across
the lanes of a slot, next to a trajectory of constant P = 6; the two-, three-, four- and a five-slot kernel class; float and
double storage.

Per batch: phase 0 with its natural exit, three fixed iterations of phase 0 (infeasible mode, the dual rows) and three fixed
iterations of phase 1 from the natural phase-0 result - ONE launch with an infeasible trajectory next to two feasible ones,
both bodies of every mode dispatch.  EVERY array of direct_ddp_batch_out_t is compared bit for bit

  * with tests/golden/scalar_stream_device.npz: the results of the library as it was BEFORE the predicated stores became
    stores through selected addresses and the mode tests left the row loops (recorded on an MI355X by
    tests/golden/make_scalar_stream_golden.py, static launch) - no f64 operation changed, so no bit may;
  * in the static launch k_iterate and in the ticket launch k_iterate_dyn, the latter with the shared line search and paired
    trials forced on (helper waves; a pair that loses a partner mid-sweep goes on in the per-trial body - that the batches
    get there is asserted from the oracle in tests/test_emu_scalar_stream.py)."""
import os

import numpy as np
import pytest

from tests import scalar_stream_lib as lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalar_stream_device.npz")
KEYS = ("DIRECT_DDP_SCHED", "DIRECT_DDP_HELP", "DIRECT_DDP_SLOTS", "DIRECT_DDP_PAIR", "DIRECT_DDP_BSHARE", "DIRECT_DDP_HALF",
        "DIRECT_DDP_CHUNK", "DIRECT_DDP_TAIL", "DIRECT_DDP_CLASSES")
FORMS = (("static", dict(DIRECT_DDP_SCHED="static"), dict(dynamic=0)),
         ("tickets", dict(DIRECT_DDP_HELP="1", DIRECT_DDP_PAIR="1"), dict(dynamic=1, shared_search=1, pair_trials=1)))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cls", list(lib.CLASSES))
def test_every_output_is_bitwise_the_recorded_one_in_both_launch_forms(built, golden, monkeypatch, cls, dt):
    for N in lib.N_CASES:
        for form, env, want in FORMS:
            for k in KEYS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            res, digest, info = lib.device_results(cls, N, dt)
            for k, v in want.items():
                assert info[k] == v, (form, N, k, info)
            assert digest == str(golden[lib.key(cls, N, dt, "inputs", "sha256")]), ("the generated inputs differ from the recorded ones", N)
            assert (res["p0fix"].fwd_passes == lib.ITERS).all() and (res["p1fix"].fwd_passes == lib.ITERS).all()
            for solve, r in res.items():
                for f in lib.OUT_FIELDS:
                    got, rec = np.ascontiguousarray(getattr(r, f)), golden[lib.key(cls, N, dt, solve, f)]
                    assert got.dtype == rec.dtype and got.shape == rec.shape and got.tobytes() == rec.tobytes(), (form, N, solve, f)
