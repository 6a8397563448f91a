"""direct_cluster_grid_path_clear_batch at the C boundary, without a GPU: the header compiles as C, the entry point is exported and
bound, the ctypes mirrors have the C sizes and offsets, and arguments the host can judge are refused before anything touches the
handle or the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_cluster.h")
NAME = "direct_cluster_grid_path_clear_batch"


def test_library_exports_the_call(built):
    lib = solver.lib()
    assert hasattr(lib, NAME) and NAME in cluster.EXPORTS
    assert set(abi.GRID_PATH_CLEAR_OUTPUTS) == {n for n, _ in abi.GridPathClearOut._fields_}
    assert [n for n, _ in abi.GridPathClearOut._fields_] == list(abi.GRID_PATH_CLEAR_OUTPUTS)  # the binding fills the struct in this order


def test_header_compiles_as_c_and_struct_sizes_match(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%d\\n",'
                   'sizeof(direct_grid_path_clear_in_t),sizeof(direct_grid_path_clear_out_t),offsetof(direct_grid_path_clear_in_t,starts),'
                   'offsetof(direct_grid_path_clear_in_t,min_d2),offsetof(direct_grid_path_clear_in_t,penalty),'
                   'offsetof(direct_grid_path_clear_out_t,path_min_d2),DIRECT_DIST_NONE);return 0;}\n' % HEADER)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.GridPathClearIn), C.sizeof(abi.GridPathClearOut), abi.GridPathClearIn.starts.offset,
                   abi.GridPathClearIn.min_d2.offset, abi.GridPathClearIn.penalty.offset, abi.GridPathClearOut.path_min_d2.offset,
                   cluster.DIST_NONE]


def _valid_structs(keep):
    """a well-formed host-memory call: 2 queries, a table of 4 entries, the codes alone asked for"""
    starts, goals = np.zeros((2, 3), np.int32), np.ones((2, 3), np.int32)
    pen, rtn = np.array([0.5, 0.25, 0.125, 0.0]), np.zeros(2, np.int32)
    keep += [starts, goals, pen, rtn]
    cin = abi.GridPathClearIn(batch=2, path_capacity=16, max_rounds=0, mem=abi.MEM_HOST, starts=starts.ctypes.data, goals=goals.ctypes.data,
                              min_d2=1, n_penalty=4, penalty=pen.ctypes.data)
    cout = abi.GridPathClearOut(rtn=rtn.ctypes.data)
    return cin, cout


def _call(cin, cout, handle=True):
    lib = cluster._lib()
    fake = C.create_string_buffer(1 << 16)  # a zeroed stand-in: no map, no field, max_batch 0
    st = lib.direct_cluster_grid_path_clear_batch(C.addressof(fake) if handle else None, None if cin is None else C.addressof(cin),
                                                  None if cout is None else C.addressof(cout))
    return st, lib.direct_cluster_last_error().decode()


def test_null_arguments_are_refused(built):
    keep = []
    cin, cout = _valid_structs(keep)
    assert _call(cin, cout, handle=False)[0] == abi.DIRECT_ERR_INVALID
    assert _call(None, cout)[0] == abi.DIRECT_ERR_INVALID
    assert _call(cin, None)[0] == abi.DIRECT_ERR_INVALID
    st, msg = _call(cin, cout)  # well-formed arguments reach the checks of the handle, which holds nothing
    assert st == abi.DIRECT_ERR_INVALID and "max_batch" in msg


@pytest.mark.parametrize("what,word", [("starts", "null"), ("goals", "null"), ("batch", "batch"), ("path_capacity", "path_capacity"),
                                       ("max_rounds", "max_rounds"), ("mem", "mem"), ("min_d2", "min_d2"), ("n_neg", "n_penalty"),
                                       ("n_big", "n_penalty"), ("null_table", "NULL penalty"), ("nan", "penalty entries"),
                                       ("inf", "penalty entries"), ("negative", "penalty entries")])
def test_host_side_validation(built, what, word):
    """the arguments alone decide these, and the message names the argument: the refusal is not the empty handle's"""
    keep = []
    cin, cout = _valid_structs(keep)
    if what in ("starts", "goals"):
        setattr(cin, what, None)
    elif what in ("batch", "path_capacity"):
        setattr(cin, what, 0)
    elif what == "max_rounds":
        cin.max_rounds = -1
    elif what == "mem":
        cin.mem = 2
    elif what == "min_d2":
        cin.min_d2 = -1
    elif what == "n_neg":
        cin.n_penalty = -1
    elif what == "n_big":
        big = np.zeros(abi.GRID_PATH_MAX_PENALTY + 1)
        keep.append(big)
        cin.n_penalty, cin.penalty = len(big), big.ctypes.data
    elif what == "null_table":
        cin.penalty = None
    else:
        keep[2][2] = {"nan": np.nan, "inf": np.inf, "negative": -1e-300}[what]
    st, msg = _call(cin, cout)
    assert st == abi.DIRECT_ERR_INVALID and word in msg, msg


def test_a_null_table_with_no_entries_and_a_full_table_pass_the_argument_checks(built):
    keep = []
    cin, cout = _valid_structs(keep)
    cin.n_penalty, cin.penalty = 0, None
    assert "max_batch" in _call(cin, cout)[1]
    full = np.zeros(abi.GRID_PATH_MAX_PENALTY)
    cin.n_penalty, cin.penalty = len(full), full.ctypes.data
    assert "max_batch" in _call(cin, cout)[1]
