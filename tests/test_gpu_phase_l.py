"""Phase L of the DDP knots on the device (tests/phase_l_lib.py): horizons of 1, 2, 3 and 7 segments, plane counts that
change from knot to knot on every boundary of the per-lane index and predicate words, next to a trajectory of constant
P = 6; two-, three-, four- and a five-slot kernel class, float and double storage.

Per batch: phase 0 with its natural exit, three fixed iterations of phase 0 (infeasible mode, the dual rows) and three fixed
iterations of phase 1 from the natural phase-0 result.  EVERY array of direct_ddp_batch_out_t is compared bit for bit

  * with tests/golden/phase_l_device.npz: the results of the library as it was BEFORE phase L's address arithmetic was
    rewritten (recorded on an MI355X by tests/golden/make_phase_l_golden.py, static launch) - no f64 operation changed, so
    no bit may;
  * between the static launch k_iterate and the ticket launch k_iterate_dyn of the same build, the latter with the shared
    line search and paired trials forced on (helper waves enter a round at phase L; a pair that loses a partner goes on in
    the per-trial body, which starts from phase L as well)."""
import os

import numpy as np
import pytest

from tests import phase_l_lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_l_device.npz")
KEYS = ("DIRECT_DDP_SCHED", "DIRECT_DDP_HELP", "DIRECT_DDP_SLOTS", "DIRECT_DDP_PAIR", "DIRECT_DDP_BSHARE", "DIRECT_DDP_HALF",
        "DIRECT_DDP_CHUNK", "DIRECT_DDP_TAIL", "DIRECT_DDP_CLASSES")
FORMS = (("static", dict(DIRECT_DDP_SCHED="static"), dict(dynamic=0)),
         ("tickets", dict(DIRECT_DDP_HELP="1", DIRECT_DDP_PAIR="1"), dict(dynamic=1, shared_search=1, pair_trials=1)))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cls", list(phase_l_lib.CLASSES))
def test_every_output_is_bitwise_the_recorded_one_in_both_launch_forms(built, golden, monkeypatch, cls, dt):
    for N in phase_l_lib.N_CASES:
        for form, env, want in FORMS:
            for k in KEYS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            res, digest, info = phase_l_lib.device_results(cls, N, dt)
            for k, v in want.items():
                assert info[k] == v, (form, N, k, info)
            assert digest == str(golden[phase_l_lib.key(cls, N, dt, "inputs", "sha256")]), ("the generated inputs differ from the recorded ones", N)
            assert (res["p0fix"].fwd_passes == phase_l_lib.ITERS).all() and (res["p1fix"].fwd_passes == phase_l_lib.ITERS).all()
            for solve, r in res.items():
                for f in phase_l_lib.OUT_FIELDS:
                    got, rec = np.ascontiguousarray(getattr(r, f)), golden[phase_l_lib.key(cls, N, dt, solve, f)]
                    assert got.dtype == rec.dtype and got.shape == rec.shape and got.tobytes() == rec.tobytes(), (form, N, solve, f)
