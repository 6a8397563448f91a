"""direct_cluster_set_unknown_policy, direct_cluster_get_unknown_policy and direct_cluster_get_open_map at the C boundary, without a
GPU: the header compiles as C99 with the two policy values, the entry points are exported and bound with struct-free signatures,
and on a zeroed buffer handed over as a handle - which means policy DIRECT_UNKNOWN_FREE and no open map - every refusal comes by
its message with no byte of the buffer written.  What needs a handle with voxels is asked by tests/test_gpu_unknown_policy.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from direct_amd import abi, cluster, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_cluster.h")
SIGNATURES = {
    "direct_cluster_set_unknown_policy": "direct_cluster_handle_t h, int32_t policy",
    "direct_cluster_get_unknown_policy": "direct_cluster_handle_t h, int32_t* policy, int64_t* stats2",
    "direct_cluster_get_open_map": "direct_cluster_handle_t h, int32_t mem, uint8_t* out",
}
ARGTYPES = {
    "direct_cluster_set_unknown_policy": [C.c_void_p, C.c_int32],
    "direct_cluster_get_unknown_policy": [C.c_void_p, C.c_void_p, C.c_void_p],
    "direct_cluster_get_open_map": [C.c_void_p, C.c_int32, C.c_void_p],
}


def _fake():
    return C.create_string_buffer(1 << 16)   # a zeroed stand-in: policy FREE, no map, no open map, 0 voxels


def test_library_exports_the_calls(built):
    lib = cluster._lib()
    for name, argtypes in ARGTYPES.items():
        assert hasattr(solver.lib(), name) and name in cluster.EXPORTS, name
        assert list(getattr(lib, name).argtypes) == argtypes, name
    for method in ("set_unknown_policy", "unknown_policy", "open_map"):
        assert callable(getattr(cluster.ClusterGenerator, method))
    assert (cluster.UNKNOWN_FREE, cluster.UNKNOWN_OCCUPIED) == (0, 1) and cluster.UNKNOWN_POLICIES == ("free", "occupied")


def test_signatures_are_struct_free_and_the_header_compiles_as_c99(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in SIGNATURES.items():
        m = re.search(r"direct_status_t %s\(([^)]*)\);" % name, text)
        assert m and " ".join(m.group(1).split()) == args, name
    src = tmp_path / "pol.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(void){printf("%%d %%d\\n",DIRECT_UNKNOWN_FREE,DIRECT_UNKNOWN_OCCUPIED);return 0;}\n' % HEADER)
    exe = tmp_path / "pol"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"0", b"1"]


def test_null_and_invalid_policies_are_refused_and_nothing_is_written(built):
    lib = cluster._lib()
    err = lambda: lib.direct_cluster_last_error().decode()
    fake = _fake()
    h = C.addressof(fake)
    for value in (cluster.UNKNOWN_FREE, cluster.UNKNOWN_OCCUPIED, 2):
        assert lib.direct_cluster_set_unknown_policy(None, value) == abi.DIRECT_ERR_INVALID and "null" in err()
    for value in (-1, 2, 3, 256, 2 ** 31 - 1, -2 ** 31):
        assert lib.direct_cluster_set_unknown_policy(h, value) == abi.DIRECT_ERR_INVALID and "policy" in err(), value
    assert bytes(fake.raw) == bytes(1 << 16)   # nothing was written into the stand-in


def test_the_getters_on_a_zeroed_handle(built):
    lib = cluster._lib()
    err = lambda: lib.direct_cluster_last_error().decode()
    fake = _fake()
    h = C.addressof(fake)
    policy = C.c_int32(-7)
    stats = np.full(2, -5, np.int64)
    assert lib.direct_cluster_get_unknown_policy(None, C.addressof(policy), stats.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_get_unknown_policy(h, None, stats.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert policy.value == -7 and (stats == -5).all()
    assert lib.direct_cluster_get_unknown_policy(h, C.addressof(policy), None) == abi.DIRECT_OK and policy.value == cluster.UNKNOWN_FREE
    policy.value = -7
    assert lib.direct_cluster_get_unknown_policy(h, C.addressof(policy), stats.ctypes.data) == abi.DIRECT_OK
    assert policy.value == cluster.UNKNOWN_FREE and stats.tolist() == [0, 0]    # FREE and zeros
    buf = np.full(8, 9, np.uint8)
    assert lib.direct_cluster_get_open_map(None, abi.MEM_HOST, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_get_open_map(h, abi.MEM_HOST, None) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_get_open_map(h, 2, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "mem" in err()
    assert lib.direct_cluster_get_open_map(h, abi.MEM_HOST, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "the handle has no open map" in err()
    assert lib.direct_cluster_get_open_map(h, abi.MEM_DEVICE, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "the handle has no open map" in err()
    assert (buf == 9).all()
    assert bytes(fake.raw) == bytes(1 << 16)
