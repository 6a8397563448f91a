"""direct_traj_audit_batch at the C boundary, without a GPU: both entry points are exported and bound, the ctypes mirrors have
the C sizes, and arguments the host can judge are refused before anything touches the handle or the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from direct_amd import abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_ddp.h")
NAMES = ("direct_traj_audit_batch", "direct_traj_audit_last_ms")


def test_library_exports_the_audit(built):
    lib = solver.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in solver.EXPORTS
    assert lib.direct_ddp_abi_version() == 1
    assert set(abi.AUDIT_OUTPUTS) == {n for n, _ in abi.AuditOut._fields_} - {"status"}
    assert (abi.AUDIT_VEL, abi.AUDIT_ACC, abi.AUDIT_JERK, abi.AUDIT_CORRIDOR, abi.AUDIT_INVALID) == (1, 2, 4, 8, 256)


def test_struct_sizes_and_bits_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%d %%d %%d %%d %%d\\n",'
                   'sizeof(direct_audit_in_t),sizeof(direct_audit_out_t),offsetof(direct_audit_in_t,clearance),'
                   'offsetof(direct_audit_out_t,best),DIRECT_AUDIT_VEL,DIRECT_AUDIT_ACC,DIRECT_AUDIT_JERK,DIRECT_AUDIT_CORRIDOR,'
                   'DIRECT_AUDIT_INVALID);return 0;}\n' % HEADER)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.AuditIn), C.sizeof(abi.AuditOut), abi.AuditIn.clearance.offset, abi.AuditOut.best.offset,
                   abi.AUDIT_VEL, abi.AUDIT_ACC, abi.AUDIT_JERK, abi.AUDIT_CORRIDOR, abi.AUDIT_INVALID]


def _valid_structs(keep):
    """a well-formed host-memory call: 2 rows of 3 segments with a corridor of 4 planes, cost, and a few outputs"""
    n_seg = np.array([3, 3], np.int32)
    T = np.ones((2, 3))
    bez = np.zeros((2, 3, 18))
    n_planes = np.full((2, 3), 4, np.int32)
    planes = np.zeros((2, 3, 4, 4))
    cost = np.zeros(2)
    status = np.zeros(2, np.int32)
    vpeak, cpeak = np.zeros(2), np.zeros(2)
    best = np.zeros(1, np.int64)
    keep += [n_seg, T, bez, n_planes, planes, cost, status, vpeak, cpeak, best]
    cin, cout = abi.AuditIn(), abi.AuditOut()
    cin.batch, cin.n_seg_max, cin.p_max, cin.mem = 2, 3, 4, abi.MEM_HOST
    cin.n_seg, cin.T, cin.bez = n_seg.ctypes.data, T.ctypes.data, bez.ctypes.data
    cin.n_planes, cin.planes, cin.cost = n_planes.ctypes.data, planes.ctypes.data, cost.ctypes.data
    cin.max_vel, cin.max_acc, cin.max_jerk, cin.clearance = 2.0, 2.0, 10.0, 0.05
    cout.status, cout.vpeak, cout.cpeak, cout.best = status.ctypes.data, vpeak.ctypes.data, cpeak.ctypes.data, best.ctypes.data
    return cin, cout


def test_null_handle_and_structs_are_refused(built):
    lib = solver.lib()
    keep = []
    cin, cout = _valid_structs(keep)
    assert lib.direct_traj_audit_batch(None, C.addressof(cin), C.addressof(cout)) == abi.DIRECT_ERR_INVALID
    assert len(lib.direct_ddp_last_error()) > 0
    ms = C.c_float()
    assert lib.direct_traj_audit_last_ms(None, C.addressof(ms)) == abi.DIRECT_ERR_INVALID
    # the argument checks come before the handle is used: a zeroed stand-in is never read
    fake = C.create_string_buffer(1 << 16)
    h = C.addressof(fake)
    assert lib.direct_traj_audit_batch(h, None, C.addressof(cout)) == abi.DIRECT_ERR_INVALID
    assert lib.direct_traj_audit_batch(h, C.addressof(cin), None) == abi.DIRECT_ERR_INVALID
    assert lib.direct_traj_audit_last_ms(h, None) == abi.DIRECT_ERR_INVALID


def _refused(edit):
    lib = solver.lib()
    keep = []
    cin, cout = _valid_structs(keep)
    edit(cin, cout, keep)
    fake = C.create_string_buffer(1 << 16)
    return lib.direct_traj_audit_batch(C.addressof(fake), C.addressof(cin), C.addressof(cout)) == abi.DIRECT_ERR_INVALID


@pytest.mark.parametrize("what", ["batch", "n_seg_max", "mem", "n_seg", "T", "status", "both", "neither", "planes_only",
                                  "n_planes_only", "p_max", "cpeak_free", "c_where_free", "velnan", "accnan", "jerknan",
                                  "clearneg", "clearnan", "on_norm", "best_without_cost"])
def test_host_side_validation(built, what):
    def edit(cin, cout, keep):
        if what in ("batch", "n_seg_max"):
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
        elif what == "planes_only":
            cin.n_planes = None
        elif what == "n_planes_only":
            cin.planes = None
        elif what == "p_max":
            cin.p_max = 0
        elif what in ("cpeak_free", "c_where_free"):
            cin.planes = cin.n_planes = None
            if what == "c_where_free":
                w = np.zeros((2, 2), np.int32)
                keep.append(w)
                cout.cpeak, cout.c_where = None, w.ctypes.data
        elif what in ("velnan", "accnan", "jerknan"):
            setattr(cin, {"velnan": "max_vel", "accnan": "max_acc", "jerknan": "max_jerk"}[what], float("nan"))
        elif what == "clearneg":
            cin.clearance = -1e-9
        elif what == "clearnan":
            cin.clearance = float("nan")
        elif what == "on_norm":
            cin.limit_on_norm = 2
        elif what == "best_without_cost":
            cin.cost = None
    assert _refused(edit)
