"""direct_cluster_map_integrate_scan_evidence, direct_cluster_get_evidence, direct_cluster_set_evidence and
direct_cluster_evidence_phase_ms at the C boundary, without a GPU: the header compiles as C99, the entry points are exported and
bound, the ctypes mirror has the C size and offsets, and every refusal a zeroed buffer handed over as a handle can reach comes in its
stated order, by its message, with no byte of the buffer written.  A zeroed handle has a map of 0 x 0 x 0 voxels, so no origin lies
inside it: the plain scan's refusals up to that one are answered here with every evidence field wrong as well, which shows that they
come first.  The refusals behind it need a handle with voxels: tests/test_gpu_evidence.py asks them of the library, and
tests/test_evidence_restatement.py asks their order of the function the library calls."""
import ctypes as C
import os
import subprocess

import numpy as np

from direct_amd import abi, cluster, solver
from tests import map_scan_harness as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_cluster.h")
NAMES = ("direct_cluster_map_integrate_scan_evidence", "direct_cluster_get_evidence", "direct_cluster_set_evidence",
         "direct_cluster_evidence_phase_ms")
FIELDS = ("scan", "hit", "miss", "ev_min", "ev_max", "occ", "reserved")


def test_library_exports_the_calls(built):
    lib = solver.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in cluster.EXPORTS, name
    assert [n for n, _ in cluster.MapEvidence._fields_] == list(FIELDS)
    for method in ("integrate_scan_evidence", "evidence_grid", "set_evidence", "evidence_phase_ms"):
        assert callable(getattr(cluster.ClusterGenerator, method))
    assert len(cluster.EVIDENCE_STATS) == 12 and cluster.EVIDENCE_STATS[:8] == cluster.SCAN_STATS


def test_header_compiles_as_c99_and_struct_layout_matches(tmp_path):
    args = ["sizeof(direct_map_evidence_t)", "sizeof(direct_map_scan_t)"] + ["offsetof(direct_map_evidence_t,%s)" % n for n in FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%s\\n",%s);return 0;}\n'
                   % (HEADER, " ".join(["%zu"] * len(args)), ",".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cluster.MapEvidence), C.sizeof(cluster.MapScan)] + [getattr(cluster.MapEvidence, n).offset for n in FIELDS]
    assert got == want
    assert got == [144, 112, 0, 112, 116, 120, 124, 128, 132]


def _fake():
    return C.create_string_buffer(1 << 16)   # a zeroed stand-in: no map, no scan grid, no evidence grid, 0 voxels


def _par(scan=None, ev=None):
    s = dict(lower=sh.LOWER, upper=sh.UPPER, res=sh.RES, max_range=1.5, origin=sh.ORIGIN, inflate=(0, 0, 0), mode=cluster.SCAN_CONTINUE,
             stride=3, flags=0)
    s.update(scan or {})
    e = dict(hit=17, miss=8, ev_min=-40, ev_max=70, occ=1, reserved=(0, 0, 0))
    e.update(ev or {})
    ms = cluster.MapScan((C.c_double * 3)(*s["lower"]), (C.c_double * 3)(*s["upper"]), s["res"], s["max_range"], (C.c_double * 3)(*s["origin"]),
                         (C.c_int32 * 3)(*s["inflate"]), s["mode"], s["stride"], s["flags"])
    return cluster.MapEvidence(ms, e["hit"], e["miss"], e["ev_min"], e["ev_max"], e["occ"], (C.c_int32 * 3)(*e["reserved"]))


def test_scan_refusals_come_first_and_in_the_plain_order(built):
    """each case is wrong in ONE way beyond those behind it in the order, and in every evidence field throughout"""
    lib = cluster._lib()
    fake = _fake()
    h = C.addressof(fake)
    pts = np.zeros((4, 3), np.float32)
    stats = np.full(12, -5, np.int64)
    bad_ev = dict(hit=0, miss=0, ev_min=1, ev_max=0, occ=0, reserved=(1, 1, 1))
    nan = float("nan")

    def call(handle=h, par=True, n=4, mem=abi.MEM_HOST, xyz=True, **scan):
        p = _par(scan, bad_ev)
        st = lib.direct_cluster_map_integrate_scan_evidence(handle, C.addressof(p) if par else None, n, mem, pts.ctypes.data if xyz else None,
                                                            stats.ctypes.data)
        return st, lib.direct_cluster_last_error().decode()

    everything = dict(mode=7, flags=2, stride=5, res=0.0, max_range=-1.0, lower=(nan, 0, 0), inflate=(-1, 0, 0))
    drop = lambda d, *keys: {k: v for k, v in d.items() if k not in keys}
    for kw, word in ((dict(handle=None, **everything), "null"), (dict(par=False), "null"),
                     (dict(n=-1, mem=9, **everything), "n_points negative"), (dict(xyz=False, mem=9, **everything), "n_points negative"),
                     (dict(mem=9, **everything), "mem"),
                     (dict(**everything), "unknown mode"),
                     (dict(**drop(everything, "mode")), "unknown flags"),
                     (dict(**drop(everything, "mode", "flags")), "stride must be 3 or 4"),
                     (dict(**drop(everything, "mode", "flags", "stride")), "resolution must be finite and positive"),
                     (dict(**drop(everything, "mode", "flags", "stride", "res")), "max_range must be finite and positive"),
                     (dict(lower=(nan, 0, 0), inflate=(-1, 0, 0)), "map_lower / map_upper must be finite"),
                     (dict(inflate=(-1, 0, 0)), "inflate must not be negative"),
                     (dict(inflate=(65, 0, 0), max_range=1e9, mode=cluster.SCAN_ADOPT), "the origin lies outside the map"),
                     (dict(), "the origin lies outside the map")):
        st, msg = call(**kw)
        assert st == abi.DIRECT_ERR_INVALID and word in msg, (kw, msg)
        for field in ("hit", "miss", "ev_min", "ev_max", "occ", "reserved"):
            assert not msg.startswith(field + " "), (kw, msg)
    assert (stats == -5).all()
    assert bytes(fake.raw) == bytes(1 << 16)   # nothing was written into the stand-in


def test_getter_setter_and_phase_refusals(built):
    lib = cluster._lib()
    err = lambda: lib.direct_cluster_last_error().decode()
    fake = _fake()
    h = C.addressof(fake)
    buf = np.zeros(8, np.int8)
    ms = np.full(5, -1, np.float32)
    assert lib.direct_cluster_get_evidence(None, abi.MEM_HOST, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_get_evidence(h, abi.MEM_HOST, None) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_get_evidence(h, 2, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "mem" in err()
    assert lib.direct_cluster_get_evidence(h, abi.MEM_HOST, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "no evidence grid" in err()
    assert lib.direct_cluster_set_evidence(None, abi.MEM_HOST, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_set_evidence(h, -1, buf.ctypes.data) == abi.DIRECT_ERR_INVALID and "mem" in err()
    assert lib.direct_cluster_evidence_phase_ms(None, ms.ctypes.data) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_evidence_phase_ms(h, None) == abi.DIRECT_ERR_INVALID and "null" in err()
    assert lib.direct_cluster_evidence_phase_ms(h, ms.ctypes.data) == abi.DIRECT_ERR_INVALID and "no timed evidence scan" in err()
    assert (ms == -1).all() and not buf.any()
    assert bytes(fake.raw) == bytes(1 << 16)


def test_the_plain_scan_still_refuses_every_flag_above_bit_0(built):
    lib = cluster._lib()
    fake = _fake()
    pts = np.zeros((4, 3), np.float32)
    for flags in (2, 3):
        p = _par(dict(flags=flags)).scan
        st = lib.direct_cluster_map_integrate_scan(C.addressof(fake), C.addressof(p), 4, abi.MEM_HOST, pts.ctypes.data, None)
        assert st == abi.DIRECT_ERR_INVALID and "unknown flags" in lib.direct_cluster_last_error().decode()
    assert bytes(fake.raw) == bytes(1 << 16)
