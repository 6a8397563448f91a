"""direct_cluster_view_gain_batch at the C boundary, without a GPU: the header compiles as C99, the entry point is exported and
bound, the ctypes mirrors have the C sizes and offsets, and every refusal comes in its stated order, by its message, on a zeroed
buffer handed over as a handle, of which no byte is written."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from direct_amd import abi, cluster, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "direct_cluster.h")
NAME = "direct_cluster_view_gain_batch"
IN_FIELDS = ("range_vox", "n", "n_dirs", "n_sets", "mem_in", "mem")
IO_FIELDS = ("voxel", "set", "dirs", "code", "gain", "seen", "ends")


def test_library_exports_the_call(built):
    assert hasattr(solver.lib(), NAME) and NAME in cluster.EXPORTS
    assert [n for n, _ in cluster.ViewGainIn._fields_] == list(IN_FIELDS)
    assert [n for n, _ in cluster.ViewGainIO._fields_] == list(IO_FIELDS)
    assert callable(cluster.ClusterGenerator.view_gain) and callable(cluster.view_directions)


def test_header_compiles_as_c99_and_struct_layouts_match(tmp_path):
    args = ["sizeof(direct_view_gain_in_t)", "sizeof(direct_view_gain_io_t)"]
    args += ["(size_t)DIRECT_VIEW_OK", "(size_t)DIRECT_VIEW_OUTSIDE", "(size_t)DIRECT_VIEW_OCCUPIED", "(size_t)DIRECT_VIEW_BAD_SET"]
    args += ["offsetof(direct_view_gain_in_t,%s)" % n for n in IN_FIELDS]
    args += ["offsetof(direct_view_gain_io_t,%s)" % n for n in IO_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%s\\n",%s);return 0;}\n'
                   % (HEADER, " ".join(["%zu"] * len(args)), ",".join(args)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cluster.ViewGainIn), C.sizeof(cluster.ViewGainIO)]
    want += [cluster.VIEW_OK, cluster.VIEW_OUTSIDE, cluster.VIEW_OCCUPIED, cluster.VIEW_BAD_SET]
    want += [getattr(cluster.ViewGainIn, n).offset for n in IN_FIELDS]
    want += [getattr(cluster.ViewGainIO, n).offset for n in IO_FIELDS]
    assert got == want
    assert got[:6] == [32, 56, 0, 1, 2, 3]


def test_refusals_in_their_order(built):
    """each case is wrong in ONE way beyond those behind it in the order, so the message shows which check came first; the zeroed
    handle answers "no map" to everything that gets that far"""
    lib = cluster._lib()
    fake = C.create_string_buffer(1 << 16)   # a zeroed stand-in: no map, no known grid
    h = C.addressof(fake)
    vox, sets, dirs = np.zeros((8, 3), np.int32), np.zeros(8, np.int32), np.ones((2, 5, 3), np.float32)
    outs = [np.full(8, -5, np.int32), np.full(8, -5, np.int32), np.full(8, -5, np.int32), np.full((8, 4), -5, np.int32)]

    def call(handle=h, cin=True, cio=True, voxel=True, directions=True, outputs=True, **field):
        v = dict(range_vox=10.0, n=8, n_dirs=5, n_sets=2, mem_in=abi.MEM_HOST, mem=abi.MEM_HOST)
        v.update(field)
        par = cluster.ViewGainIn(*[v[k] for k in IN_FIELDS])
        io = cluster.ViewGainIO(vox.ctypes.data if voxel else None, sets.ctypes.data, dirs.ctypes.data if directions else None,
                                *[a.ctypes.data if outputs else None for a in outs])
        st = lib.direct_cluster_view_gain_batch(handle, C.addressof(par) if cin else None, C.addressof(io) if cio else None)
        return st, lib.direct_cluster_last_error().decode()

    INV, UNS = abi.DIRECT_ERR_INVALID, abi.DIRECT_ERR_UNSUPPORTED
    worse = dict(mem_in=7, mem=9, n=-1, n_dirs=0, n_sets=0, range_vox=-1.0, voxel=False, directions=False, outputs=False)
    drop = lambda *keys: {k: v for k, v in worse.items() if k not in keys}
    cases = (
        (dict(handle=None, **worse), INV, "null"), (dict(cin=False), INV, "null"), (dict(cio=False, **worse), INV, "null"),       # 1
        (dict(**worse), INV, "mem"), (dict(**drop("mem_in")), INV, "mem"),                                                       # 2
        (dict(**drop("mem_in", "mem")), INV, "n must not be negative"),                                                          # 3
        (dict(**drop("mem_in", "mem", "n")), INV, "n_dirs must be at least 1"),
        (dict(**drop("mem_in", "mem", "n", "n_dirs")), INV, "n_sets must be at least 1"),
        (dict(range_vox=-1.0, voxel=False, directions=False, outputs=False), INV, "range_vox must be finite and positive"),      # 4
        (dict(range_vox=0.0, voxel=False), INV, "range_vox must be finite and positive"),
        (dict(range_vox=math.nan, voxel=False), INV, "range_vox must be finite and positive"),
        (dict(range_vox=math.inf, voxel=False), INV, "range_vox must be finite and positive"),
        (dict(voxel=False, directions=False, outputs=False, range_vox=49.0), INV, "null voxel or dirs"),                         # 5
        (dict(directions=False, outputs=False, range_vox=49.0), INV, "null voxel or dirs"),
        (dict(outputs=False, range_vox=49.0, n_dirs=65537), INV, "no output"),
        (dict(range_vox=49.0, n_dirs=65537), UNS, "range_vox"),                                                                  # 6
        (dict(range_vox=1e300), UNS, "range_vox"),
        (dict(n_dirs=65537), UNS, "n_dirs above"),
        (dict(range_vox=48.99, n_dirs=65536), INV, "no map"),                                                                    # 7
        (dict(n=0, voxel=False, directions=False, outputs=False), INV, "no map"),     # n == 0 needs no array, and still a map
        (dict(), INV, "no map"),
    )
    for kw, status, word in cases:
        st, msg = call(**kw)
        assert st == status and word in msg, (kw, st, msg)
        assert word == "no map" or "no map" not in msg
    assert all((a == -5).all() for a in outs)
    assert bytes(fake.raw) == bytes(1 << 16)   # nothing was written into the stand-in


def test_view_directions():
    d = cluster.view_directions(8, 3, -0.5, 0.5)
    assert d.dtype == np.float32 and d.shape == (24, 3) and np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    az, el = np.arctan2(d[:, 1], d[:, 0]).reshape(8, 3), np.arcsin(d[:, 2]).reshape(8, 3)
    assert np.allclose(el, np.array([-1, 0, 1]) / 3.0, atol=1e-6)                            # cell centres, azimuth major
    assert np.allclose(az[:, 0], -np.pi + (np.arange(8) + 0.5) * np.pi / 4, atol=1e-6)      # a full turn without a doubled ray
    fov = cluster.view_directions(5, 1, 0.0, 0.0, -0.3, 0.3, yaw=1.0)
    assert np.allclose(np.arctan2(fov[:, 1], fov[:, 0]), 1.0 + np.array([-0.24, -0.12, 0.0, 0.12, 0.24]), atol=1e-6) and not fov[:, 2].any()
    turned = cluster.view_directions(5, 1, 0.0, 0.0, -0.3 + 1.0, 0.3 + 1.0)
    assert np.allclose(fov, turned, atol=1e-6)
    assert np.stack([fov, turned]).shape == (2, 5, 3)
