"""direct_cluster_free_components, direct_cluster_get_free_components and direct_cluster_reachable_batch at the C boundary,
without a GPU: the header compiles as C99, the entry points are exported and bound, the ctypes mirrors have the C sizes and
offsets, and every refusal the arguments alone decide comes, by its message, before anything touches the handle or the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_cluster.h")
NAMES = ("direct_cluster_free_components", "direct_cluster_get_free_components", "direct_cluster_reachable_batch")
IN_FIELDS = ("n", "mem_in", "min_d2", "starts", "goals")
OUT_FIELDS = ("mem", "reserved") + abi.REACHABLE_OUTPUTS


def test_library_exports_the_calls(built):
    lib = solver.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in cluster.EXPORTS, name
    assert [n for n, _ in abi.ReachableIn._fields_] == list(IN_FIELDS)
    assert [n for n, _ in abi.ReachableOut._fields_] == list(OUT_FIELDS)
    for method in ("build_free_components", "free_components", "reachable"):
        assert callable(getattr(cluster.ClusterGenerator, method))


def test_header_compiles_as_c99_and_struct_layouts_match(tmp_path):
    fmt = " ".join(["%zu"] * (2 + len(IN_FIELDS) + len(OUT_FIELDS)))
    args = ["sizeof(direct_reachable_in_t)", "sizeof(direct_reachable_out_t)"]
    args += ["offsetof(direct_reachable_in_t,%s)" % n for n in IN_FIELDS]
    args += ["offsetof(direct_reachable_out_t,%s)" % n for n in OUT_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%s\\n",%s);return 0;}\n'
                   % (HEADER, fmt, ",".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.ReachableIn), C.sizeof(abi.ReachableOut)]
    want += [getattr(abi.ReachableIn, n).offset for n in IN_FIELDS]
    want += [getattr(abi.ReachableOut, n).offset for n in OUT_FIELDS]
    assert got == want
    assert got[:2] == [32, 32]


def _valid_structs(keep):
    """a well-formed host-memory call of 5 pairs, every output asked for"""
    starts, goals = np.zeros((5, 3), np.int32), np.ones((5, 3), np.int32)
    outs = [np.zeros(5, np.int32) for _ in abi.REACHABLE_OUTPUTS]
    keep += [starts, goals] + outs
    cin = abi.ReachableIn(n=5, mem_in=abi.MEM_HOST, min_d2=0, starts=starts.ctypes.data, goals=goals.ctypes.data)
    cout = abi.ReachableOut(abi.MEM_HOST, 0, *[a.ctypes.data for a in outs])
    return cin, cout


def _fake():
    return C.create_string_buffer(1 << 16)   # a zeroed stand-in: no map, no field, no labels


def _reach(cin, cout, handle=True):
    lib = cluster._lib()
    fake = _fake()
    st = lib.direct_cluster_reachable_batch(C.addressof(fake) if handle else None, None if cin is None else C.addressof(cin),
                                            None if cout is None else C.addressof(cout))
    return st, lib.direct_cluster_last_error().decode()


def test_null_arguments_are_refused(built):
    keep = []
    cin, cout = _valid_structs(keep)
    assert _reach(cin, cout, handle=False)[0] == abi.DIRECT_ERR_INVALID
    assert _reach(None, cout)[0] == abi.DIRECT_ERR_INVALID
    assert _reach(cin, None)[0] == abi.DIRECT_ERR_INVALID
    st, msg = _reach(cin, cout)   # well-formed arguments reach the checks of the handle, which holds nothing
    assert st == abi.DIRECT_ERR_INVALID and "no map" in msg, msg
    cout.rtn = cout.goal_label = cout.goal_size = None   # every output may be NULL
    cin.min_d2 = 7
    assert "no map" in _reach(cin, cout)[1]


@pytest.mark.parametrize("what,word", [("starts", "null"), ("goals", "null"), ("n_zero", "n must be positive"), ("n_neg", "n must be positive"),
                                       ("mem_in", "mem"), ("mem", "mem"), ("min_d2", "min_d2 must not be negative")])
def test_reachable_host_side_validation(built, what, word):
    """the arguments alone decide these, and the message names the argument: the refusal is not the empty handle's"""
    keep = []
    cin, cout = _valid_structs(keep)
    if what in ("starts", "goals"):
        setattr(cin, what, None)
    elif what == "n_zero":
        cin.n = 0
    elif what == "n_neg":
        cin.n = -4
    elif what == "mem_in":
        cin.mem_in = 2
    elif what == "mem":
        cout.mem = -1
    elif what == "min_d2":
        cin.min_d2 = -1
    st, msg = _reach(cin, cout)
    assert st == abi.DIRECT_ERR_INVALID and word in msg and "no map" not in msg, msg


def test_build_and_fetch_validation(built):
    lib = cluster._lib()
    err = lambda: lib.direct_cluster_last_error().decode()
    fake = _fake()
    h = C.addressof(fake)
    stats = np.zeros(4, np.int64)
    assert lib.direct_cluster_free_components(None, 0, stats.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_free_components(h, -1, stats.ctypes.data) == abi.DIRECT_ERR_INVALID and "min_d2 must not be negative" in err()
    for floor in (0, 1, 2, 100):   # well-formed: the empty handle's refusal
        assert lib.direct_cluster_free_components(h, floor, None) == abi.DIRECT_ERR_INVALID and "no map" in err()
    buf, built_with = np.zeros(8, np.int32), C.c_int32(0)
    assert lib.direct_cluster_get_free_components(None, abi.MEM_HOST, buf.ctypes.data, None, None) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_get_free_components(h, 2, buf.ctypes.data, None, None) == abi.DIRECT_ERR_INVALID and "mem" in err()
    assert lib.direct_cluster_get_free_components(h, abi.MEM_HOST, None, None, C.addressof(built_with)) == abi.DIRECT_ERR_INVALID and "no map" in err()
    assert bytes(fake.raw) == bytes(1 << 16)   # nothing was written into the stand-in
