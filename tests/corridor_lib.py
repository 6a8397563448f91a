"""What the tests of the three corridor calls (direct_cluster_cube_corridor_batch, direct_cluster_cube_corridor_clear_batch,
direct_cluster_corridor_batch) share - TEST INFRASTRUCTURE of tests/test_gpu_cube_corridor.py, tests/test_gpu_cube_corridor_clear.py,
tests/test_gpu_cluster_corridor.py, the stride tests and the CPU tests of the harnesses: the byte comparison, the 40 rows, the raw
C-ABI call of the edge tests, the bystander snapshot, the chain into direct_ddp_plan_batch and the run of a C++ mirror.  Each call's
own assertions stay in its test."""
import contextlib
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from direct_amd import abi, cluster, devmem, solver
from tests import cube_corridor_harness as ch

RES, LOWER = ch.RES, ch.LOWER


def same(a, b, keys):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def to_host(r):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def pick(r, at, keys):
    return {k: r[k][at] for k in keys}


# ---- the rows ---------------------------------------------------------------------------------------------------------------

def named_rows():
    """the 15 paths of the named cases that lie inside the map"""
    paths = [np.asarray(p, np.int32) for c in ch.named_cases() if c["name"] != "outside_voxel" for p in c["paths"]]
    assert len(paths) == 15
    return paths


def rows40():
    """the named cases inside the map, then random walks (seed 9): 40 rows on the crafted map"""
    named = named_rows()
    return named + ch.random_paths(ch.crafted_map(), 40 - len(named), seed=9)


# ---- the raw C-ABI call of the edge tests -----------------------------------------------------------------------------------

NAN, INF = float("nan"), float("inf")
# what every corridor call refuses with DIRECT_ERR_INVALID: overrides of RawCall.call
INVALID = [dict(h=C.c_void_p(None)), dict(null_in=True), dict(null_out=True), dict(path_xyz=None), dict(path_len=None), dict(batch=0),
           dict(batch=-1), dict(path_capacity=0), dict(seg_capacity=0), dict(itr_inflate_max=0), dict(p_max=5), dict(mem_in=2), dict(omem=2),
           dict(plane_dtype=2), dict(resolution=0.0), dict(resolution=-0.2), dict(resolution=NAN), dict(resolution=INF),
           dict(map_lower=(C.c_double * 3)(0.0, NAN, 0.0))]


class RawCall:
    """One corridor entry point on host memory with every output pre-filled with 77s.  entry(h, in pointer, out pointer, **rest)
    places the arguments of the C function; In, Out: its structs; keys: the output arrays in the order of Out; extras: further
    arrays the call writes (info, stats), which untouched() watches as well; fields: In's fields beyond the common ones"""

    def __init__(self, gen, entry, In, Out, keys, xyz, n, seg_capacity, p_max, extras=(), **fields):
        B, S, P = len(n), int(seg_capacity), int(p_max)
        shapes = dict(n_seg=(B,), n_planes=(B, S), planes=(B, S, P, 4), seeds=(B, S, 3), centers=(B, S, 3), cube_idx=(B, S, 6), rtn=(B,))
        self.out = {k: np.full(shapes[k], 77, np.float64 if k in ("planes", "seeds", "centers") else np.int32) for k in keys}
        self.gen, self.entry, self.In, self.Out, self.keys, self.extras = gen, entry, In, Out, keys, extras
        self.fields = dict(batch=B, path_capacity=xyz.shape[1], mem_in=abi.MEM_HOST, itr_inflate_max=1000, path_xyz=xyz.ctypes.data,
                           path_len=n.ctypes.data, pop_back=1, seg_capacity=S, p_max=P, plane_dtype=abi.F64, resolution=RES,
                           map_lower=(C.c_double * 3)(*LOWER), **fields)
        self.keep = [v.copy() for v in self._watched()]

    def _watched(self):
        return list(self.out.values()) + list(self.extras)

    def call(self, h=None, null_in=False, null_out=False, omem=abi.MEM_HOST, outputs=None, **kw):
        """overrides: h, a NULL in / out struct, the output memory kind, other output arrays (a missing key is a NULL pointer), any
        field of In; whatever else is given goes to entry()"""
        par = self.In(**self.fields)
        rest = {}
        for k, v in kw.items():
            if hasattr(par, k):
                setattr(par, k, v)
            else:
                rest[k] = v
        outputs = self.out if outputs is None else outputs
        o = self.Out(omem, 0, *[outputs[k].ctypes.data if k in outputs else None for k in self.keys])
        return self.entry(self.gen.h if h is None else h, None if null_in else C.addressof(par), None if null_out else C.addressof(o), **rest)

    def untouched(self):
        return all(a.tobytes() == b.tobytes() for a, b in zip(self._watched(), self.keep))

    def only_codes(self, **kw):
        """the call with every output but rtn NULL -> (status, rtn)"""
        only = np.full(len(self.out["rtn"]), -1, np.int32)
        return self.call(outputs=dict(rtn=only), **kw), only


@contextlib.contextmanager
def handle_without_map():
    fresh = cluster.ClusterGenerator(ch.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)
    try:
        yield fresh
    finally:
        fresh.close()


# ---- what a corridor call must leave alone ----------------------------------------------------------------------------------

class Bystanders:
    """Taken before a corridor call on a handle that holds ch.crafted_map() and a valid distance field: resident clusters (seen
    through hull_planes), a host and a device grid-path result, the field and the map.  check() after the call asserts that all
    are what they were.  dev_path may serve as the call's input."""
    SEEDS = np.array([[5, 5, 5], [20, 3, 3], [13, 4, 4], [15, 12, 5]], np.int32)
    STARTS, GOALS = np.array([[5, 5, 5], [1, 1, 1]], np.int32), np.array([[22, 18, 10], [20, 12, 5]], np.int32)

    def __init__(self, gen):
        self.gen = gen
        self.field = gen.distance_field()
        self.path = gen.grid_paths(self.STARTS, self.GOALS, path_capacity=64, want_dist=True)
        self.dev_path = gen.grid_paths(self.STARTS, self.GOALS, path_capacity=64, mem="device")
        self.dev_keep = {k: v.clone() for k, v in self.dev_path.items()}
        gen.polygon_generation(self.SEEDS, 1000, 0, fetch_clusters=False)
        self.hull = self._hull()
        gen.polygon_generation(self.SEEDS, 1000, 0, fetch_clusters=False)

    def _hull(self):
        return self.gen.hull_planes(RES, LOWER, batch=len(self.SEEDS), plane_capacity=64, vertex_capacity=64)

    def check(self):
        gen, want, got = self.gen, self.hull, self._hull()
        assert (want["rtn"] == cluster.HULL_OK).all()
        for k in ("rtn", "n_planes", "n_vertices", "degenerate", "center"):
            assert np.array_equal(want[k], got[k]), k
        for b in range(len(self.SEEDS)):
            assert np.array_equal(want["planes"][b], got["planes"][b]) and np.array_equal(want["vertices"][b], got["vertices"][b])
        for k, v in self.dev_path.items():
            assert v.cpu().numpy().tobytes() == self.dev_keep[k].cpu().numpy().tobytes(), k
        assert np.array_equal(gen.distance_field(), self.field)   # still valid, still the same
        again = gen.grid_paths(self.STARTS, self.GOALS, path_capacity=64, want_dist=True)
        assert (self.path["rtn"] == cluster.GRID_PATH_OK).all() and np.array_equal(again["path_len"], self.path["path_len"])
        assert all(np.array_equal(a, b) for a, b in zip(again["paths"], self.path["paths"]))
        assert np.array_equal(gen.get_map(), ch.crafted_map())


# ---- the chain into the optimiser ---------------------------------------------------------------------------------------------

def chain_ends(paths, pick):
    """-> (x0, xd) [B][9] on the device: the centres of the first and the last voxel of the device-resident paths `pick` selects"""
    import torch
    dev = paths["path_xyz"].device
    centre = lambda v: v.to(torch.float64) * RES + 0.5 * RES + torch.from_numpy(LOWER).to(dev)
    last = (paths["path_len"][pick] - 1).long()
    x0, xd = torch.zeros((len(pick), 9), dtype=torch.float64, device=dev), torch.zeros((len(pick), 9), dtype=torch.float64, device=dev)
    x0[:, :3] = centre(paths["path_xyz"][pick, 0])
    xd[:, :3] = centre(paths["path_xyz"][pick, last])
    return x0, xd


def plan_chain(cor, x0, xd, N, P):
    """direct_ddp_plan_batch on the device tensors n_seg, n_planes, planes, seeds of `cor` and x0, xd, with T0 = NULL, against the
    same call on their host copies: both phases, seven fields, byte for byte.  The plumbing and the layout are under test, not
    the solver -> (the host copies, (phase 0, phase 1) from host memory, (phase 0, phase 1) from device memory)"""
    import torch
    B, dev = x0.shape[0], "cuda:0"
    t = dict(n_seg=cor["n_seg"].contiguous(), x0=x0, xd=xd, n_planes=cor["n_planes"].contiguous(), planes=cor["planes"].contiguous(),
             seeds=cor["seeds"].contiguous())
    cin = abi.BatchIn()
    cin.batch, cin.n_seg_max, cin.p_max, cin.mem = B, N, P, abi.MEM_DEVICE
    for k, v in t.items():
        setattr(cin, k, v.data_ptr())
    p0, p1 = abi.phase0_params(iter_max=20), abi.phase1_params(iter_max=20)
    s = solver.DdpSolver(B, N, P, np.float64, device=0)
    o0, o1 = devmem.DeviceResult(B, N, np.float64, dev), devmem.DeviceResult(B, N, np.float64, dev)
    torch.cuda.synchronize()
    s.plan_device(p0, p1, cin, o0.cout, o1.cout)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in t.items()}
    hb = abi.HostBatch(h["n_seg"], h["x0"], h["xd"], np.zeros((B, N)), h["n_planes"], h["planes"], seeds=h["seeds"]).without_T0()
    r0, r1 = s.plan(p0, p1, hb)
    s.close()
    d0, d1 = o0.to_host(), o1.to_host()
    for dv, hv in ((d0, r0), (d1, r1)):
        for k in ("rtn", "iter_used", "fwd_passes", "cost", "T", "bez", "poly"):
            assert np.asarray(getattr(dv, k)).tobytes() == np.asarray(getattr(hv, k)).tobytes(), k
    return h, (r0, r1), (d0, d1)


# ---- the C++ mirrors ------------------------------------------------------------------------------------------------------------

def run_cpp_mirror(workdir, source, rows, tail=b"", args=()):
    """compiles tests/cpp/<source> against the built library and runs it on in.bin: the map's geometry, the rows as voxel centres,
    the crafted map, then `tail`; args follow the file on the command line.  The program compares for itself: it must exit with 0"""
    fin, exe = os.path.join(str(workdir), "in.bin"), os.path.join(str(workdir), "gen")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3id3di", *ch.DIMS, RES, *LOWER, len(rows)))
        for p in rows:
            f.write(struct.pack("<i", len(p)))
            f.write(np.ascontiguousarray(p.astype(np.float64) * RES + 0.5 * RES + LOWER, np.float64).tobytes())
        f.write(ch.crafted_map().tobytes())
        f.write(tail)
    lib = os.path.dirname(solver.LIB_PATH)
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ch.ROOT, "tests", "cpp", source), "-o", exe, "-L" + lib, "-ldirect_ddp",
                           "-Wl,-rpath," + lib + ":/opt/rocm/lib"])
    out = subprocess.run([exe, fin] + [str(a) for a in args], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
