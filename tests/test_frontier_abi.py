"""direct_cluster_frontier, direct_cluster_get_known, direct_cluster_set_known and the flags of direct_cluster_map_integrate_scan at
the C boundary, without a GPU: the header compiles as C99, the entry points are exported and bound, the ctypes mirrors have the C
sizes and offsets, and every refusal comes in its stated order, by its message, on a zeroed buffer handed over as a handle, of which
no byte is written."""
import ctypes as C
import os
import subprocess

import numpy as np

from direct_amd import abi, cluster, solver
from tests import map_scan_harness as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_cluster.h")
NAMES = ("direct_cluster_frontier", "direct_cluster_get_known", "direct_cluster_set_known")
IN_FIELDS = ("min_d2", "min_size", "capacity", "mem")
OUT_FIELDS = ("label", "size", "centroid", "rep", "voxel_label", "stats")
SCAN_FIELDS = ("map_lower", "map_upper", "resolution", "max_range", "origin", "inflate", "mode", "stride", "flags")


def test_library_exports_the_calls(built):
    lib = solver.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in cluster.EXPORTS, name
    assert [n for n, _ in cluster.FrontierIn._fields_] == list(IN_FIELDS)
    assert [n for n, _ in cluster.FrontierOut._fields_] == list(OUT_FIELDS)
    assert [n for n, _ in cluster.MapScan._fields_] == list(SCAN_FIELDS)
    for method in ("known_grid", "set_known", "frontiers"):
        assert callable(getattr(cluster.ClusterGenerator, method))


def test_header_compiles_as_c99_and_struct_layouts_match(tmp_path):
    args = ["sizeof(direct_frontier_in_t)", "sizeof(direct_frontier_out_t)", "sizeof(direct_map_scan_t)", "(size_t)DIRECT_SCAN_TRACK_KNOWN"]
    args += ["offsetof(direct_frontier_in_t,%s)" % n for n in IN_FIELDS]
    args += ["offsetof(direct_frontier_out_t,%s)" % n for n in OUT_FIELDS]
    args += ["offsetof(direct_map_scan_t,%s)" % n for n in SCAN_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%s\\n",%s);return 0;}\n'
                   % (HEADER, " ".join(["%zu"] * len(args)), ",".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cluster.FrontierIn), C.sizeof(cluster.FrontierOut), C.sizeof(cluster.MapScan), cluster.SCAN_TRACK_KNOWN]
    want += [getattr(cluster.FrontierIn, n).offset for n in IN_FIELDS]
    want += [getattr(cluster.FrontierOut, n).offset for n in OUT_FIELDS]
    want += [getattr(cluster.MapScan, n).offset for n in SCAN_FIELDS]
    assert got == want
    assert got[:4] == [16, 48, 112, 1] and got[-1] == 108   # flags keeps the offset and size `reserved` had


def _fake():
    return C.create_string_buffer(1 << 16)   # a zeroed stand-in: no map, no known grid, no field


def test_frontier_refusals_in_their_order(built):
    """each case is wrong in ONE way beyond those behind it in the order, so the message shows which check came first; the zeroed
    handle answers the last three"""
    lib = cluster._lib()
    fake = _fake()
    h = C.addressof(fake)
    arrays = [np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros((8, 3), np.int32), np.zeros((8, 3), np.int32)]
    stats = np.full(6, -5, np.int64)

    def call(handle=h, cin=True, cout=True, outputs=True, **field):
        v = dict(min_d2=0, min_size=1, capacity=8, mem=abi.MEM_HOST)
        v.update(field)
        par = cluster.FrontierIn(v["min_d2"], v["min_size"], v["capacity"], v["mem"])
        o = cluster.FrontierOut(*([a.ctypes.data for a in arrays] if outputs else [None] * 4), None, stats.ctypes.data)
        st = lib.direct_cluster_frontier(handle, C.addressof(par) if cin else None, C.addressof(o) if cout else None)
        return st, lib.direct_cluster_last_error().decode()

    bad_everywhere = dict(mem=7, min_d2=-1, min_size=0, capacity=-1)
    for kw, word in ((dict(handle=None, **bad_everywhere), "null"), (dict(cin=False), "null"), (dict(cout=False, **bad_everywhere), "null"),
                     (dict(**bad_everywhere), "mem"),                                              # 2 before 3
                     (dict(min_d2=-1, min_size=0, capacity=-1), "min_d2 must not be negative"),    # 3, in the order of the text
                     (dict(min_size=0, capacity=-1), "min_size must be at least 1"),
                     (dict(capacity=-1, outputs=False), "capacity must not be negative"),
                     (dict(outputs=False), "capacity without a per-component output"),             # 4 before 5
                     (dict(), "no map"),                                                           # 5 before 6 and 7
                     (dict(min_d2=9), "no map"),
                     (dict(capacity=0, outputs=False), "no map")):                                 # a count-only call is well-formed
        st, msg = call(**kw)
        assert st == abi.DIRECT_ERR_INVALID and word in msg, (kw, msg)
        assert word == "no map" or "no map" not in msg
    assert (stats == -5).all() and not any(a.any() for a in arrays)
    assert bytes(fake.raw) == bytes(1 << 16)   # nothing was written into the stand-in


def test_known_grid_calls_and_the_scan_flags(built):
    lib = cluster._lib()
    err = lambda: lib.direct_cluster_last_error().decode()
    fake = _fake()
    h = C.addressof(fake)
    buf = np.zeros(8, np.uint8)
    assert lib.direct_cluster_get_known(None, abi.MEM_HOST, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_get_known(h, abi.MEM_HOST, None) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_get_known(h, 2, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "mem" in err()
    assert lib.direct_cluster_get_known(h, abi.MEM_HOST, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "no known grid" in err()
    assert lib.direct_cluster_set_known(None, abi.MEM_HOST, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_set_known(h, -1, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "mem" in err()
    pts = np.zeros((4, 3), np.float32)
    for flags, word in ((2, "unknown flags"), (3, "unknown flags"), (-1, "unknown flags"), (1 << 31 - 1, "unknown flags")):
        p = cluster.MapScan((C.c_double * 3)(*sh.LOWER), (C.c_double * 3)(*sh.UPPER), sh.RES, 1.5, (C.c_double * 3)(*sh.ORIGIN),
                            (C.c_int32 * 3)(0, 0, 0), cluster.SCAN_CONTINUE, 3, flags)
        assert lib.direct_cluster_map_integrate_scan(h, C.addressof(p), 4, abi.MEM_HOST, pts.ctypes.data, None) == abi.DIRECT_ERR_INVALID
        assert word in err(), (flags, err())
    assert bytes(fake.raw) == bytes(1 << 16)
