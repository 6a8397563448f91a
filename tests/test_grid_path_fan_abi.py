"""direct_cluster_grid_path_fan_batch at the C boundary, without a GPU: the header compiles as C99, the entry point is exported and
bound, the ctypes mirrors have the C sizes and offsets, and every refusal the arguments alone decide comes, by its message, before
anything touches the handle or the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_cluster.h")
NAME = "direct_cluster_grid_path_fan_batch"
IN_FIELDS = ("n_src", "n_goal", "path_capacity", "max_rounds", "mem", "sources", "goals", "goal_src", "min_d2", "n_penalty", "penalty")


def test_library_exports_the_call(built):
    lib = solver.lib()
    assert hasattr(lib, NAME) and NAME in cluster.EXPORTS
    assert [n for n, _ in abi.GridPathFanOut._fields_] == list(abi.GRID_PATH_FAN_OUTPUTS)  # the binding fills the struct in this order
    assert [n for n, _ in abi.GridPathFanIn._fields_] == list(IN_FIELDS)


def test_header_compiles_as_c99_and_struct_layouts_match(tmp_path):
    fmt = " ".join(["%zu"] * (2 + len(IN_FIELDS) + len(abi.GRID_PATH_FAN_OUTPUTS)))
    args = ["sizeof(direct_grid_path_fan_in_t)", "sizeof(direct_grid_path_fan_out_t)"]
    args += ["offsetof(direct_grid_path_fan_in_t,%s)" % n for n in IN_FIELDS]
    args += ["offsetof(direct_grid_path_fan_out_t,%s)" % n for n in abi.GRID_PATH_FAN_OUTPUTS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%s\\n",%s);return 0;}\n'
                   % (HEADER, fmt, ",".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.GridPathFanIn), C.sizeof(abi.GridPathFanOut)]
    want += [getattr(abi.GridPathFanIn, n).offset for n in IN_FIELDS]
    want += [getattr(abi.GridPathFanOut, n).offset for n in abi.GRID_PATH_FAN_OUTPUTS]
    assert got == want
    assert got[:2] == [64, 64]


def _valid_structs(keep, clear=True):
    """a well-formed host-memory call: 2 sources, 5 goals, (clear) a floor and a table of 4 entries, the codes alone asked for"""
    sources, goals = np.zeros((2, 3), np.int32), np.ones((5, 3), np.int32)
    gs = np.array([0, 1, 1, 0, 1], np.int32)
    pen, rtn, aux = np.array([0.5, 0.25, 0.125, 0.0]), np.zeros(5, np.int32), np.zeros(5 * 16, np.int32)
    keep += [sources, goals, pen, rtn, gs, aux]
    cin = abi.GridPathFanIn(n_src=2, n_goal=5, path_capacity=16, max_rounds=0, mem=abi.MEM_HOST, sources=sources.ctypes.data,
                            goals=goals.ctypes.data, goal_src=gs.ctypes.data, min_d2=2 if clear else 0, n_penalty=4 if clear else 0,
                            penalty=pen.ctypes.data if clear else None)
    cout = abi.GridPathFanOut(rtn=rtn.ctypes.data)
    return cin, cout


def _call(cin, cout, handle=True):
    lib = cluster._lib()
    fake = C.create_string_buffer(1 << 16)  # a zeroed stand-in: no map, no field, max_batch 0
    st = lib.direct_cluster_grid_path_fan_batch(C.addressof(fake) if handle else None, None if cin is None else C.addressof(cin),
                                                None if cout is None else C.addressof(cout))
    return st, lib.direct_cluster_last_error().decode()


def test_null_arguments_are_refused(built):
    keep = []
    cin, cout = _valid_structs(keep)
    assert _call(cin, cout, handle=False)[0] == abi.DIRECT_ERR_INVALID
    assert _call(None, cout)[0] == abi.DIRECT_ERR_INVALID
    assert _call(cin, None)[0] == abi.DIRECT_ERR_INVALID
    for clear in (True, False):
        cin, cout = _valid_structs(keep, clear)
        st, msg = _call(cin, cout)  # well-formed arguments reach the checks of the handle, which holds nothing
        assert st == abi.DIRECT_ERR_INVALID and "max_batch" in msg, msg


@pytest.mark.parametrize("what,word", [("sources", "null"), ("goals", "null"), ("n_src", "n_src must be positive"),
                                       ("n_src_neg", "n_src must be positive"), ("n_goal", "n_goal must be positive"),
                                       ("path_capacity", "path_capacity"), ("max_rounds", "max_rounds"), ("mem", "mem"),
                                       ("min_d2", "min_d2"), ("n_neg", "n_penalty"), ("n_big", "n_penalty"), ("null_table", "NULL penalty"),
                                       ("nan", "penalty entries"), ("inf", "penalty entries"), ("negative", "penalty entries"),
                                       ("null_goal_src", "NULL goal_src"), ("goal_src_low", "goal_src entry"),
                                       ("goal_src_high", "goal_src entry"), ("neutral_d2", "neutral mode"), ("neutral_min", "neutral mode"),
                                       ("neutral_floor_1", "neutral mode")])
def test_host_side_validation(built, what, word):
    """the arguments alone decide these, and the message names the argument: the refusal is not the empty handle's"""
    keep = []
    cin, cout = _valid_structs(keep, clear=not what.startswith("neutral"))
    if what in ("sources", "goals"):
        setattr(cin, what, None)
    elif what in ("n_src", "n_goal", "path_capacity"):
        setattr(cin, what, 0)
    elif what == "n_src_neg":
        cin.n_src = -3
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
    elif what in ("nan", "inf", "negative"):
        keep[2][2] = {"nan": np.nan, "inf": np.inf, "negative": -1e-300}[what]
    elif what == "null_goal_src":
        cin.goal_src = None   # with n_src == 2
    elif what == "goal_src_low":
        keep[4][3] = -1
    elif what == "goal_src_high":
        keep[4][4] = 2
    elif what == "neutral_d2":
        cout.path_d2 = keep[5].ctypes.data
    elif what == "neutral_min":
        cout.path_min_d2 = keep[5].ctypes.data
    elif what == "neutral_floor_1":
        cin.min_d2, cout.path_min_d2 = 1, keep[5].ctypes.data   # min_d2 = 1 without a table is neutral mode too
    st, msg = _call(cin, cout)
    assert st == abi.DIRECT_ERR_INVALID and word in msg, msg


def test_well_formed_variants_pass_the_argument_checks(built):
    """a NULL goal_src with one source, clear-mode outputs in clear mode, a full table, a floor alone: all reach the handle's checks"""
    keep = []
    cin, cout = _valid_structs(keep)
    cin.n_src, cin.goal_src = 1, None
    cout.path_d2 = cout.path_min_d2 = keep[5].ctypes.data
    assert "max_batch" in _call(cin, cout)[1]
    full = np.zeros(abi.GRID_PATH_MAX_PENALTY)
    cin.n_penalty, cin.penalty = len(full), full.ctypes.data
    assert "max_batch" in _call(cin, cout)[1]
    cin.n_penalty, cin.penalty, cin.min_d2 = 0, None, 2
    assert "max_batch" in _call(cin, cout)[1]
