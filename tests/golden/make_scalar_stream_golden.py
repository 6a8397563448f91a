"""Records tests/golden/scalar_stream_device.npz: every output array of the batches of tests/scalar_stream_lib.py as the
DEVICE computes them (static launch), for tests/test_gpu_scalar_stream.py.

The file on record was made on an MI355X with the library of the commit BEFORE the lane predicates and the mode dispatch of
the knot loops were rewritten (built from that commit and passed in DIRECT_DDP_LIB); the rewrite touches no f64 operation, so
the test asks for the same bits.  Run it again only when the solver's results are meant to change, from the repository root:

    python tests/golden/make_scalar_stream_golden.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import scalar_stream_lib  # noqa: E402


def main(out):
    os.environ["DIRECT_DDP_SCHED"] = "static"
    rec = {}
    for cls in scalar_stream_lib.CLASSES:
        for N in scalar_stream_lib.N_CASES:
            for dt in (np.float32, np.float64):
                res, digest, info = scalar_stream_lib.device_results(cls, N, dt)
                assert info["dynamic"] == 0, info
                rec[scalar_stream_lib.key(cls, N, dt, "inputs", "sha256")] = np.array(digest)
                for solve, r in res.items():
                    for f in scalar_stream_lib.OUT_FIELDS:
                        rec[scalar_stream_lib.key(cls, N, dt, solve, f)] = np.ascontiguousarray(getattr(r, f))
                print(cls, N, np.dtype(dt).name, "rtn", res["p0"].rtn, "infeas_out", res["p0"].infeas_out,
                      "p1fix cost", res["p1fix"].cost, flush=True)
    np.savez_compressed(out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out, len(rec), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "scalar_stream_device.npz"))
