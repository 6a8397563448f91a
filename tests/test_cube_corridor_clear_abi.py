"""direct_cluster_cube_corridor_clear_batch at the C boundary, without a GPU: the header compiles as C99 with the declaration in
it, the entry point is exported and bound, and every refusal the arguments alone decide comes, by its message, before anything
touches the handle or the device - the plain call's refusals through this entry point and the negative floor."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_cluster.h")
NAME = "direct_cluster_cube_corridor_clear_batch"


def test_library_exports_the_call(built):
    lib = solver.lib()
    assert hasattr(lib, NAME) and NAME in cluster.EXPORTS
    assert cluster._lib().direct_cluster_cube_corridor_clear_batch.argtypes == list(abi.CUBE_CORRIDOR_CLEAR_ARGTYPES)


def test_header_declares_the_call_in_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include "%s"\n'
                   'typedef direct_status_t (*fn_t)(direct_cluster_handle_t, const direct_cube_corridor_in_t*, int32_t,\n'
                   '                                direct_cube_corridor_out_t*, int64_t*);\n'
                   'fn_t take(void) { return %s; }\n' % (HEADER, NAME))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "decl.o")])


def _call(min_d2=4, handle=True, null_in=False, null_out=False, omem=abi.MEM_HOST, **kw):
    lib = cluster._lib()
    fake = C.create_string_buffer(1 << 16)  # a zeroed stand-in: no map, no field
    xyz, n, rtn, info = np.zeros((2, 8, 3), np.int32), np.full(2, 8, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.int64)
    par = abi.CubeCorridorIn(batch=2, path_capacity=8, mem_in=abi.MEM_HOST, itr_inflate_max=1000, path_xyz=xyz.ctypes.data,
                             path_len=n.ctypes.data, pop_back=1, seg_capacity=8, p_max=6, plane_dtype=abi.F64, resolution=0.2,
                             map_lower=(C.c_double * 3)(0.0, 0.0, 0.0))
    for k, v in kw.items():
        setattr(par, k, v)
    o = abi.CubeCorridorOut(omem, 0, None, None, None, None, None, None, rtn.ctypes.data)
    st = lib.direct_cluster_cube_corridor_clear_batch(C.addressof(fake) if handle else None, None if null_in else C.addressof(par), min_d2,
                                                      None if null_out else C.addressof(o), info.ctypes.data)
    assert rtn.tolist() == [77, 77] and info.tolist() == [77, 77]
    return st, lib.direct_cluster_last_error().decode()


@pytest.mark.parametrize("min_d2", [0, 1, 2, 9])
def test_well_formed_arguments_reach_the_handle(built, min_d2):
    st, msg = _call(min_d2)
    assert st == abi.DIRECT_ERR_INVALID and "no map" in msg, msg


@pytest.mark.parametrize("kw,word", [(dict(handle=False), "null"), (dict(null_in=True), "null"), (dict(null_out=True), "null"),
                                     (dict(path_xyz=None), "null"), (dict(path_len=None), "null"), (dict(batch=0), "batch"),
                                     (dict(path_capacity=0), "path_capacity"), (dict(seg_capacity=-1), "seg_capacity"),
                                     (dict(itr_inflate_max=0), "itr_inflate_max"), (dict(p_max=5), "p_max"), (dict(mem_in=2), "mem"),
                                     (dict(omem=2), "mem"), (dict(plane_dtype=2), "plane_dtype"), (dict(resolution=0.0), "resolution"),
                                     (dict(resolution=float("nan")), "resolution"),
                                     (dict(map_lower=(C.c_double * 3)(0.0, float("inf"), 0.0)), "map_lower"),
                                     (dict(min_d2=-1), "min_d2"), (dict(min_d2=-2 ** 31), "min_d2")])
def test_host_side_validation(built, kw, word):
    """the arguments alone decide these, and the message names the argument: the refusal is not the empty handle's"""
    st, msg = _call(**kw)
    assert st == abi.DIRECT_ERR_INVALID and word in msg and "no map" not in msg, msg
