"""direct_traj_eval_batch at the C boundary, without a GPU: both entry points are exported and bound, the ctypes mirrors
have the C sizes, and arguments the host can judge are refused before anything touches the handle or the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from direct_amd import abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_ddp.h")
NAMES = ("direct_traj_eval_batch", "direct_traj_eval_last_ms")


def test_library_exports_the_evaluation(built):
    lib = solver.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in solver.EXPORTS
    assert lib.direct_ddp_abi_version() == 1
    assert set(abi.EVAL_OUTPUTS) == {n for n, _ in abi.EvalOut._fields_} - {"status"}


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n",'
                   'sizeof(direct_eval_in_t),sizeof(direct_eval_out_t),offsetof(direct_eval_in_t,t0),'
                   'offsetof(direct_eval_out_t,state));return 0;}\n' % HEADER)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(abi.EvalIn), C.sizeof(abi.EvalOut), abi.EvalIn.t0.offset, abi.EvalOut.state.offset]


def _valid_structs(keep):
    """a well-formed host-memory call: 2 rows of 3 segments, 4 explicit times, every output"""
    n_seg = np.array([3, 3], np.int32)
    T = np.ones((2, 3))
    bez = np.zeros((2, 3, 18))
    t = np.zeros((2, 4))
    status = np.zeros(2, np.int32)
    pos = np.zeros((2, 4, 3))
    keep += [n_seg, T, bez, t, status, pos]
    cin, cout = abi.EvalIn(), abi.EvalOut()
    cin.batch, cin.n_seg_max, cin.m_max, cin.mem = 2, 3, 4, abi.MEM_HOST
    cin.n_seg, cin.T, cin.bez, cin.t = n_seg.ctypes.data, T.ctypes.data, bez.ctypes.data, t.ctypes.data
    cout.status, cout.pos = status.ctypes.data, pos.ctypes.data
    return cin, cout


def test_null_handle_and_structs_are_refused(built):
    lib = solver.lib()
    keep = []
    cin, cout = _valid_structs(keep)
    assert lib.direct_traj_eval_batch(None, C.addressof(cin), C.addressof(cout)) == abi.DIRECT_ERR_INVALID
    assert len(lib.direct_ddp_last_error()) > 0
    ms = C.c_float()
    assert lib.direct_traj_eval_last_ms(None, C.addressof(ms)) == abi.DIRECT_ERR_INVALID
    # the argument checks come before the handle is used: a zeroed stand-in is never read
    fake = C.create_string_buffer(1 << 16)
    h = C.addressof(fake)
    assert lib.direct_traj_eval_batch(h, None, C.addressof(cout)) == abi.DIRECT_ERR_INVALID
    assert lib.direct_traj_eval_batch(h, C.addressof(cin), None) == abi.DIRECT_ERR_INVALID
    assert lib.direct_traj_eval_last_ms(h, None) == abi.DIRECT_ERR_INVALID


def _refused(edit):
    lib = solver.lib()
    keep = []
    cin, cout = _valid_structs(keep)
    edit(cin, cout, keep)
    fake = C.create_string_buffer(1 << 16)
    return lib.direct_traj_eval_batch(C.addressof(fake), C.addressof(cin), C.addressof(cout)) == abi.DIRECT_ERR_INVALID


@pytest.mark.parametrize("what", ["batch", "n_seg_max", "m_max", "mem", "n_seg", "T", "status", "both", "neither",
                                  "dt0", "dtneg", "dtnan", "dtinf", "t0nan", "t0inf"])
def test_host_side_validation(built, what):
    def edit(cin, cout, keep):
        if what in ("batch", "n_seg_max", "m_max"):
            setattr(cin, what, 0)
        elif what == "mem":
            cin.mem = 2
        elif what in ("n_seg", "T"):
            setattr(cin, what, None)
        elif what == "status":
            cout.status = None
        elif what == "both":
            cin.poly = cin.bez
        elif what == "neither":
            cin.bez = None
        else:  # grid mode
            cin.t = None
            cin.t0, cin.dt = {"dt0": (0.0, 0.0), "dtneg": (0.0, -0.1), "dtnan": (0.0, float("nan")),
                              "dtinf": (0.0, float("inf")), "t0nan": (float("nan"), 0.1), "t0inf": (float("inf"), 0.1)}[what]
    assert _refused(edit)
