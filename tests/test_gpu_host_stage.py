"""The host staging layer of the batched entry points (direct_amd/csrc/host_stage.h) on the GPU: the two memory-kind pairs no
other test covers (direct_traj_sample_batch and direct_cluster_hull_planes_batch on device-resident arrays against the host
call), and one reuse sequence per handle - calls of different sizes through the handle's one staging block, each against the
same call on a fresh handle.  Everything is compared bit for bit: both sides run the same kernels on the same inputs."""
import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import map_cloud_harness as mh
from tests import plan_check_harness as ph

pytestmark = pytest.mark.gpu
SENTINEL = 7.25
RES, LOWER = 0.2, np.array([-12.0, -12.0, 0.0])
EVAL_ALL = ("t_total", "seg", "pos", "vel", "acc", "jerk", "snap", "state")


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    return torch


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same_dict(got, want, what):
    assert sorted(got) == sorted(want), what
    for k, w in want.items():
        if isinstance(w, list):
            assert len(got[k]) == len(w), (what, k)
            for b, (x, y) in enumerate(zip(got[k], w)):
                same_bits(x, y, (what, k, b))
        elif w is not None:
            same_bits(got[k], w, (what, k))


def plans(seed, B, nm, dtype, pm=0):
    """random plans: n_seg in 1 .. nm, durations, control points (and pm planes per segment that hold the origin)"""
    rng = np.random.default_rng(seed)
    d = dict(n_seg=rng.integers(1, nm + 1, B).astype(np.int32), T=rng.uniform(0.3, 0.9, (B, nm)).astype(dtype),
             bez=rng.normal(0.0, 1.0, (B, nm, 18)).astype(dtype))
    if pm:
        nrm = rng.normal(0.0, 1.0, (B, nm, pm, 3))
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        d["planes"] = np.concatenate([nrm, -rng.uniform(3.0, 6.0, (B, nm, pm, 1))], -1).astype(dtype)
        d["n_planes"] = rng.integers(1, pm + 1, (B, nm)).astype(np.int32)
    return d


# ---- direct_traj_sample_batch: device-resident arrays against the host call ---------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("with_cmax", [False, True])
def test_sample_on_device_arrays_equals_the_host_call(built, dtype, with_cmax):
    torch = _torch()
    B, nm, cap, pm = 3, 4, 64, 5
    p = plans(21, B, nm, dtype, pm)
    p["n_seg"][:] = (1, 4, 3)
    p["T"][2, 1] = -1.0                      # a negative duration: the row comes back with count == -1
    corridor = dict(n_planes=p["n_planes"], planes=p["planes"]) if with_cmax else {}
    s = solver.DdpSolver(B, nm, pm, dtype)
    host = s.sample(p["n_seg"], p["bez"], p["T"], 0.05, cap, derivs=2, **corridor)
    dev = torch.device("cuda:0")
    s.set_stream(torch.cuda.current_stream().cuda_stream)
    up = {k: torch.from_numpy(v).to(dev) for k, v in p.items()}
    td = torch.float64 if dtype == np.float64 else torch.float32
    o = dict(count=torch.full((B,), -7, dtype=torch.int32, device=dev), seg_first=torch.full((B, nm), -7, dtype=torch.int32, device=dev))
    for k in ("pos", "vel", "acc"):
        o[k] = torch.full((B, cap, 3), SENTINEL, dtype=td, device=dev)
    for k in ("length", "vmax", "amax") + (("cmax",) if with_cmax else ()):
        o[k] = torch.full((B,), SENTINEL, dtype=td, device=dev)
    cin, cout = abi.SampleIn(), abi.SampleOut()
    cin.batch, cin.n_seg_max, cin.capacity, cin.derivs, cin.mem, cin.dt = B, nm, cap, 2, abi.MEM_DEVICE, 0.05
    cin.n_seg, cin.bez, cin.T = up["n_seg"].data_ptr(), up["bez"].data_ptr(), up["T"].data_ptr()
    if with_cmax:
        cin.p_max, cin.n_planes, cin.planes = pm, up["n_planes"].data_ptr(), up["planes"].data_ptr()
    for k, v in o.items():
        setattr(cout, k, v.data_ptr())
    s.sample_device(cin, cout)
    torch.cuda.synchronize()
    d = {k: v.cpu().numpy() for k, v in o.items()}
    s.close()
    assert sorted(d) == sorted(host)
    assert list(host["count"][:2] > 0) == [True, True] and host["count"][2] == -1 and host["count"].max() <= cap
    for k in ("count", "length", "vmax", "amax") + (("cmax",) if with_cmax else ()):
        same_bits(d[k], host[k], k)
    for b in range(B):
        c, n = max(int(host["count"][b]), 0), (int(p["n_seg"][b]) if host["count"][b] >= 0 else 0)
        same_bits(d["seg_first"][b, :n], host["seg_first"][b, :n], ("seg_first", b))
        assert (d["seg_first"][b, n:] == -7).all() and (host["seg_first"][b, n:] == 0).all(), b
        for k in ("pos", "vel", "acc"):
            same_bits(d[k][b, :c], host[k][b, :c], (k, b))
            # past count: the device arrays keep what they held, the host arrays read 0
            assert (d[k][b, c:] == SENTINEL).all() and (host[k][b, c:] == 0).all(), (k, b)


# ---- direct_cluster_hull_planes_batch: device outputs, and device voxels, against the host call ---------------------------
HULL_CASES = [np.zeros((0, 3), np.int32), np.array([[4, 4, 5]], np.int32),
              np.array([[x, y, 5] for x in range(3, 9) for y in range(4, 7)], np.int32)]   # empty, one voxel, the 6 x 3 slab


def hull_raw(gen, clusters, pcap, vcap, mem_in, mem):
    """the C call with voxels and outputs in the given memory kinds -> NumPy arrays; unwritten device entries hold -7 / SENTINEL"""
    torch = _torch()
    dev = torch.device("cuda:0")
    B = len(clusters)
    xyz, num = np.zeros((B, gen.ccap, 3), np.int32), np.zeros(B, np.int32)
    for b, c in enumerate(clusters):
        xyz[b, :len(c)] = c
        num[b] = len(c)
    shapes = (("planes", (B, pcap, 4), np.float64), ("plane_int", (B, pcap, 4), np.int64), ("n_planes", (B,), np.int32),
              ("vertices", (B, vcap, 3), np.float64), ("n_vertices", (B,), np.int32), ("center", (B, 3), np.float64),
              ("degenerate", (B,), np.int32), ("rtn", (B,), np.int32))
    fill = lambda dt: SENTINEL if dt == np.float64 else -7
    if mem == abi.MEM_DEVICE:
        out = {k: torch.full(shape, fill(dt), dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, shape, dt in shapes}
    else:
        out = {k: np.full(shape, fill(dt), dt) for k, shape, dt in shapes}
    ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
    vox = (torch.from_numpy(xyz).to(dev), torch.from_numpy(num).to(dev)) if mem_in == abi.MEM_DEVICE else (xyz, num)
    torch.cuda.synchronize()                 # the handle's stream is not torch's
    lower = np.ascontiguousarray(LOWER)
    st = cluster._lib().direct_cluster_hull_planes_batch(gen.h, B, mem_in, ptr(vox[0]), ptr(vox[1]), RES, lower.ctypes.data, pcap, vcap,
                                                         mem, *[ptr(out[k]) for k, _, _ in shapes])
    assert st == abi.DIRECT_OK, cluster._lib().direct_cluster_last_error()
    return {k: (v.cpu().numpy() if hasattr(v, "data_ptr") else v) for k, v in out.items()}


def test_hull_on_device_arrays_equals_the_host_call(built):
    gen = cluster.ClusterGenerator((16, 16, 16), max_batch=4, cluster_capacity=64, candidate_capacity=64)
    host = hull_raw(gen, HULL_CASES, 64, 128, abi.MEM_HOST, abi.MEM_HOST)
    assert list(host["rtn"]) == [cluster.HULL_FLAT, cluster.HULL_OK, cluster.HULL_OK] and (host["n_planes"][1:] >= 4).all()
    for mem_in, mem in ((abi.MEM_HOST, abi.MEM_DEVICE), (abi.MEM_DEVICE, abi.MEM_HOST), (abi.MEM_DEVICE, abi.MEM_DEVICE)):
        d = hull_raw(gen, HULL_CASES, 64, 128, mem_in, mem)
        for k in ("rtn", "n_planes", "n_vertices", "degenerate"):
            same_bits(d[k], host[k], (k, mem_in, mem))
        for b in range(len(HULL_CASES)):
            n_p, n_v, ok = int(host["n_planes"][b]), int(host["n_vertices"][b]), host["rtn"][b] == cluster.HULL_OK
            same_bits(d["planes"][b, :n_p], host["planes"][b, :n_p], ("planes", b, mem_in, mem))
            same_bits(d["plane_int"][b, :n_p], host["plane_int"][b, :n_p], ("plane_int", b, mem_in, mem))
            same_bits(d["vertices"][b, :n_v], host["vertices"][b, :n_v], ("vertices", b, mem_in, mem))
            if ok:
                same_bits(d["center"][b], host["center"][b], ("center", b, mem_in, mem))
            if mem == abi.MEM_DEVICE:        # device-resident outputs are untouched where the kernels do not write
                assert (d["planes"][b, n_p:] == SENTINEL).all() and (d["plane_int"][b, n_p:] == -7).all()
                assert (d["vertices"][b, n_v:] == SENTINEL).all() and (ok or (d["center"][b] == SENTINEL).all())
    gen.close()


# ---- one staging block per handle: calls of different sizes in a row, each against a fresh handle ---------------------------
def ddp_calls():
    a, b, c, big = plans(1, 2, 4, np.float64), plans(2, 5, 4, np.float64, pm=6), plans(3, 3, 4, np.float64), plans(4, 5, 4, np.float64)
    rng = np.random.default_rng(5)
    t8, t300 = rng.uniform(-0.2, 3.0, (2, 8)), rng.uniform(-0.2, 3.0, (5, 300))
    cost, rtn = rng.uniform(1.0, 2.0, 5), np.array([0, 0, -1, 0, 0], np.int32)
    ev_small = lambda s: s.evaluate(a["n_seg"], a["T"], bez=a["bez"], times=t8, outputs=EVAL_ALL)
    return [("eval B2 M8", ev_small),
            ("audit B5", lambda s: s.audit(b["n_seg"], b["T"], bez=b["bez"], n_planes=b["n_planes"], planes=b["planes"], max_vel=2.0,
                                           max_acc=3.0, max_jerk=50.0, clearance=0.1, cost=cost, rtn=rtn)),
            ("sample B3", lambda s: s.sample(c["n_seg"], c["bez"], c["T"], 0.1, 64, derivs=2)),
            ("eval B5 M300", lambda s: s.evaluate(big["n_seg"], big["T"], bez=big["bez"], times=t300, outputs=EVAL_ALL)),
            ("eval B2 M8 again", ev_small)]


def test_ddp_handle_reuses_its_staging_block(built):
    calls = ddp_calls()
    fresh = []
    for name, fn in calls:
        s = solver.DdpSolver(5, 4, 6, np.float64)
        fresh.append(fn(s))
        s.close()
    assert set(abi.AUDIT_OUTPUTS) <= set(fresh[1])          # the audit call asks for every output
    s = solver.DdpSolver(5, 4, 6, np.float64)
    for (name, fn), want in zip(calls, fresh):
        same_dict(fn(s), want, name)
    s.close()


def cluster_calls(grid):
    inp = ph.pick(ph.shared_inputs()["crafted"], "bez")
    free = np.argwhere(grid[:20] == 0)
    ends = free[np.random.default_rng(7).choice(len(free), 4, replace=False)].astype(np.int32)
    box = np.array([[x, y, z] for x in range(2, 6) for y in range(3, 6) for z in range(1, 4)], np.int32)
    cases = HULL_CASES + [box]

    def hull(pcap, vcap):
        def run(g):
            r = g.hull_planes(RES, LOWER, clusters=cases, plane_capacity=pcap, vertex_capacity=vcap)
            r["center"] = r["center"][r["rtn"] == cluster.HULL_OK]      # a cluster without a hull has no centre written
            return r
        return run
    return [("hull 64 / 128", hull(64, 128)),
            ("grid_path", lambda g: g.grid_paths(ends[:2], ends[2:], path_capacity=256)),
            ("plan_check", lambda g: g.check_plans(inp["n_seg"], inp["T"], ph.LOWER, ph.RES, bez=inp["bez"], depth=5)),
            ("hull 256 / 1024", hull(256, 1024))]


def test_cluster_handle_reuses_its_staging_blocks(built):
    grid = ph.shared_map()
    calls = cluster_calls(grid)

    def handle():
        g = cluster.ClusterGenerator(mh.DIMS, max_batch=4, cluster_capacity=2048, candidate_capacity=512)
        g.set_map(grid)
        return g
    fresh = []
    for name, fn in calls:
        g = handle()
        fresh.append(fn(g))
        g.close()
    assert (fresh[0]["rtn"][1:] == cluster.HULL_OK).all() and (fresh[1]["rtn"] == cluster.GRID_PATH_OK).any()
    g = handle()
    for (name, fn), want in zip(calls, fresh):
        same_dict(fn(g), want, name)
    g.close()
