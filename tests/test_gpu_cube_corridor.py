"""direct_cluster_cube_corridor_batch (include/direct_cluster.h, "cube corridors"; kernels in direct_amd/csrc/cube_corridor.h) on
the device, through the C-ABI: against the g++ build of the same arithmetic (tests/cube_corridor_harness.py, itself held against
three independent witnesses by tests/test_cube_corridor_restatement.py), against the path that exists beside it - a lock-step walk
over polygon_generation(seed, itr, 0) + hull_planes() on the same handle -, launch-shape independence, a change of map, what the
call leaves alone, the device-resident chain into direct_ddp_plan_batch, and the edges of the ABI."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, devmem, solver
from tests import cube_corridor_harness as ch

pytestmark = pytest.mark.gpu
RES, LOWER = ch.RES, ch.LOWER
KEYS = abi.CUBE_CORRIDOR_OUTPUTS
CAP, SEG = 40, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b, keys=KEYS):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("cube_corridor_gpu"))


@pytest.fixture(scope="module")
def gen(built):
    g = cluster.ClusterGenerator(ch.DIMS, max_batch=64, cluster_capacity=2100, candidate_capacity=64)
    g.set_map(ch.crafted_map())
    yield g
    g.close()


@pytest.fixture(scope="module")
def rows():
    """the paths of the named cases that lie inside the map, and random walks: 40 rows on the crafted map"""
    paths = []
    for c in ch.named_cases():
        if c["name"] != "outside_voxel":
            paths += [p for p in c["paths"]]
    paths += ch.random_paths(ch.crafted_map(), 40 - len(paths), seed=9)
    assert len(paths) == 40
    return [np.asarray(p, np.int32) for p in paths]


def to_host(r):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in r.items()}


def test_device_equals_the_harness(gen, harness, rows):
    """1.  every output, bit for bit: host and device memory, both dtypes, both walks, two resolutions; the rows beside a bad one too"""
    import torch
    grid = ch.crafted_map()
    bad = next(c for c in ch.named_cases() if c["name"] == "outside_voxel")["paths"]
    xyz, n = ch.pack_paths(rows + bad, CAP)
    for pop_back, dtype, res in ((True, np.float64, RES), (False, np.float64, RES), (True, np.float32, RES), (False, np.float32, 0.01),
                                 (True, np.float64, 0.01)):
        want = ch.corridors(harness, grid, xyz, n, res=res, pop_back=pop_back, seg_capacity=SEG, p_max=7, dtype=dtype)
        host = gen.cube_corridors(xyz, n, LOWER, res, pop_back=pop_back, seg_capacity=SEG, p_max=7, dtype=dtype)
        same(host, want)
        dev = gen.cube_corridors(torch.from_numpy(xyz).to("cuda:0"), torch.from_numpy(n).to("cuda:0"), LOWER, res, pop_back=pop_back,
                                 seg_capacity=SEG, p_max=7, dtype=dtype)
        assert all(v.is_cuda for v in dev.values())
        same(to_host(dev), want)
        assert want["rtn"][:len(rows)].tolist() == [ch.OK] * len(rows) and (want["rtn"][len(rows):] == ch.BAD_PATH).sum() == 3
    print("cube corridors of %d rows: %.3f ms, up to %d polytopes per row" % (len(n), gen.last_ms(), want["n_seg"].max()))


def lock_step_walk(gen, paths, res, pop_back, itr=1000):
    """the corridors as the parent produces them: polyhedronGenerator::walk in lock step, every round one polygon_generation(seeds,
    itr, 0) for the seeds that are due and one hull_planes() on the resident clusters"""
    def outside(cur, pl):
        return any(cur[0] * p[0] + cur[1] * p[1] + cur[2] * p[2] + p[3] > 0.01 for p in pl)

    cor = [[] for _ in paths]
    nxt, lst, codes = [0] * len(paths), [None] * len(paths), []
    while True:
        due = []
        for b, p in enumerate(paths):
            while nxt[b] < len(p):
                cur = [int(p[nxt[b]][a]) * res + 0.5 * res + float(LOWER[a]) for a in range(3)]
                if cur == lst[b]:
                    nxt[b] += 1
                    continue
                if pop_back and len(cor[b]) > 1 and not outside(cur, cor[b][-2]["planes"]):
                    cor[b].pop()
                if not cor[b] or outside(cur, cor[b][-1]["planes"]):
                    due.append((b, cur))
                    break
                lst[b] = cur
                nxt[b] += 1
        if not due:
            return cor, codes
        seeds = np.array([paths[b][nxt[b]] for b, _ in due], np.int32)
        g = gen.polygon_generation(seeds, itr_inflate_max=itr, itr_cluster_max=0, fetch_clusters=False)
        h = gen.hull_planes(res, LOWER, batch=len(due), plane_capacity=16, vertex_capacity=16)
        codes += g["rtn"].tolist() + h["rtn"].tolist()
        for i, (b, cur) in enumerate(due):
            v = g["vertex_idx"][i]
            cor[b].append(dict(planes=h["planes"][i].tolist(), n_planes=int(h["n_planes"][i]), center=h["center"][i], seed=cur,
                               cube=[v[7], v[15], v[23], v[1], v[9], v[17]]))
            lst[b] = cur
            nxt[b] += 1


@pytest.mark.parametrize("pop_back", [True, False])
def test_device_equals_the_lock_step_walk(gen, rows, pop_back):
    """2.  planes, n_planes, centres, seeds and cubes of EVERY row, bit for bit, against the existing generation + hull path; that
    path's codes are all OK (a cube's surface on this map is under 2100 voxels, a box has eight line-extreme points)"""
    xyz, n = ch.pack_paths(rows, CAP)
    got = gen.cube_corridors(xyz, n, LOWER, RES, pop_back=pop_back, seg_capacity=SEG)
    cor, codes = lock_step_walk(gen, rows, RES, pop_back)
    assert codes and not any(codes)
    assert (got["rtn"] == cluster.CUBE_CORRIDOR_OK).all()
    for b in range(len(rows)):
        k = len(cor[b])
        assert got["n_seg"][b] == k, b
        assert got["n_planes"][b, :k].tolist() == [c["n_planes"] for c in cor[b]] == [6] * k
        assert got["planes"][b, :k].tobytes() == np.array([c["planes"] for c in cor[b]], np.float64).tobytes(), b
        assert got["centers"][b, :k].tobytes() == np.array([c["center"] for c in cor[b]], np.float64).tobytes(), b
        assert got["seeds"][b, :k].tobytes() == np.array([c["seed"] for c in cor[b]], np.float64).tobytes(), b
        assert got["cube_idx"][b, :k].tolist() == [c["cube"] for c in cor[b]], b
    assert max(len(c) for c in cor) >= 4


def test_launch_shape_independence(gen, rows):
    """3.  one call of B rows, two calls of B / 2 rows and a permuted batch give identical bytes"""
    xyz, n = ch.pack_paths(rows, CAP)
    one = gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG)
    h = len(rows) // 2
    a, b = gen.cube_corridors(xyz[:h], n[:h], LOWER, RES, seg_capacity=SEG), gen.cube_corridors(xyz[h:], n[h:], LOWER, RES, seg_capacity=SEG)
    same({k: np.concatenate([a[k], b[k]]) for k in KEYS}, one)
    perm = np.random.default_rng(1).permutation(len(rows))
    p = gen.cube_corridors(xyz[perm], n[perm], LOWER, RES, seg_capacity=SEG)
    same(p, {k: one[k][perm] for k in KEYS})
    same(gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG), one)   # and the used workspace changes nothing


def test_follows_the_map_the_handle_holds(gen, harness, rows):
    """4.  after set_map with another map the same paths give that map's corridors"""
    xyz, n = ch.pack_paths(rows, CAP)
    before = gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG)
    other = ch.random_map(80, 0.08)
    try:
        gen.set_map(other)
        got = gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG)
    finally:
        gen.set_map(ch.crafted_map())
    same(got, ch.corridors(harness, other, xyz, n, seg_capacity=SEG))
    assert got["cube_idx"].tobytes() != before["cube_idx"].tobytes()
    same(gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG), before)


def test_leaves_the_rest_of_the_handle_alone(gen, rows):
    """5.  resident clusters, a grid-path result and the distance field from before the call are unchanged by it"""
    grid = ch.crafted_map()
    xyz, n = ch.pack_paths(rows, CAP)
    seeds = np.array([[5, 5, 5], [20, 3, 3], [13, 4, 4], [15, 12, 5]], np.int32)
    starts, goals = np.array([[5, 5, 5], [1, 1, 1]], np.int32), np.array([[22, 18, 10], [20, 12, 5]], np.int32)
    gen.polygon_generation(seeds, 1000, 0, fetch_clusters=False)
    want_hull = gen.hull_planes(RES, LOWER, batch=len(seeds), plane_capacity=64, vertex_capacity=64)
    want_path = gen.grid_paths(starts, goals, path_capacity=64, want_dist=True)
    dev_path = gen.grid_paths(starts, goals, path_capacity=64, mem="device")
    keep = {k: v.clone() for k, v in dev_path.items()}
    gen.build_distance_field()
    want_field = gen.distance_field()
    gen.polygon_generation(seeds, 1000, 0, fetch_clusters=False)
    gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG)
    gen.cube_corridors(dev_path["path_xyz"], dev_path["path_len"], LOWER, RES, seg_capacity=SEG)
    got_hull = gen.hull_planes(RES, LOWER, batch=len(seeds), plane_capacity=64, vertex_capacity=64)
    assert np.array_equal(gen.distance_field(), want_field)   # still valid, still the same
    assert (want_hull["rtn"] == cluster.HULL_OK).all()
    for k in ("rtn", "n_planes", "n_vertices", "degenerate", "center"):
        assert np.array_equal(want_hull[k], got_hull[k]), k
    for b in range(len(seeds)):
        assert np.array_equal(want_hull["planes"][b], got_hull["planes"][b]) and np.array_equal(want_hull["vertices"][b], got_hull["vertices"][b])
    for k, v in dev_path.items():
        assert v.cpu().numpy().tobytes() == keep[k].cpu().numpy().tobytes(), k
    again = gen.grid_paths(starts, goals, path_capacity=64, want_dist=True)
    assert (want_path["rtn"] == cluster.GRID_PATH_OK).all() and np.array_equal(again["path_len"], want_path["path_len"])
    assert all(np.array_equal(a, b) for a, b in zip(again["paths"], want_path["paths"]))
    assert np.array_equal(grid, gen.get_map())


def test_chain_on_the_device_into_the_optimiser(built):
    """6.  set_map_from_cloud -> grid_paths(mem="device") -> cube_corridors (device in, device out) -> direct_ddp_plan_batch with
    device inputs, T0 = NULL and the call's seeds gives the bytes of the same arrays passed through host memory.  The plumbing and
    the layout are under test, not the solver: no return code is asked for."""
    import torch
    dev = "cuda:0"
    N, P = 12, 6
    occupied = np.argwhere(ch.crafted_map() == 1)
    cloud = (occupied * RES + 0.5 * RES + LOWER).astype(np.float32)
    gen = cluster.ClusterGenerator(ch.DIMS, max_batch=16, cluster_capacity=64, candidate_capacity=64)
    gen.set_map_from_cloud(torch.from_numpy(cloud).to(dev), LOWER, RES, cloud_margin=0.0)
    free = np.argwhere(gen.get_map() == 0)
    rng = np.random.default_rng(6)
    starts, goals = free[rng.integers(len(free), size=16)].astype(np.int32), free[rng.integers(len(free), size=16)].astype(np.int32)
    paths = gen.grid_paths(starts, goals, path_capacity=64, mem="device")
    cor = gen.cube_corridors(paths["path_xyz"], paths["path_len"], LOWER, RES, seg_capacity=N, p_max=P)
    gen.close()
    ok = (cor["rtn"] == cluster.CUBE_CORRIDOR_OK) & (cor["n_seg"] >= 2)
    pick = torch.nonzero(ok).flatten()[:6]
    B = int(pick.numel())
    assert B >= 2, (cor["rtn"].cpu(), cor["n_seg"].cpu(), paths["rtn"].cpu())
    centre = lambda v: v.to(torch.float64) * RES + 0.5 * RES + torch.from_numpy(LOWER).to(dev)
    last = (paths["path_len"][pick] - 1).long()
    x0, xd = torch.zeros((B, 9), dtype=torch.float64, device=dev), torch.zeros((B, 9), dtype=torch.float64, device=dev)
    x0[:, :3] = centre(paths["path_xyz"][pick, 0])
    xd[:, :3] = centre(paths["path_xyz"][pick, last])
    t = dict(n_seg=cor["n_seg"][pick].contiguous(), x0=x0, xd=xd, n_planes=cor["n_planes"][pick].contiguous(),
             planes=cor["planes"][pick].contiguous(), seeds=cor["seeds"][pick].contiguous())
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
    print("chain: %d rows, n_seg %s, rtn %s" % (B, h["n_seg"].tolist(), r1.rtn.tolist()))
    for dv, hv in ((d0, r0), (d1, r1)):
        for k in ("rtn", "iter_used", "fwd_passes", "cost", "T", "bez", "poly"):
            assert np.asarray(getattr(dv, k)).tobytes() == np.asarray(getattr(hv, k)).tobytes(), k
    assert (h["n_seg"] <= N).all()


def test_abi_edges(gen, rows):
    """7.  every DIRECT_ERR_INVALID case launches nothing (the outputs keep their bytes); OVERFLOW and BAD_PATH rows beside good ones"""
    L = cluster._lib()
    xyz, n = ch.pack_paths(rows[:4], CAP)
    out = {k: np.full(s, 77, d) for k, s, d in (("n_seg", 4, np.int32), ("n_planes", (4, SEG), np.int32), ("planes", (4, SEG, 6, 4), np.float64),
                                                ("seeds", (4, SEG, 3), np.float64), ("centers", (4, SEG, 3), np.float64),
                                                ("cube_idx", (4, SEG, 6), np.int32), ("rtn", 4, np.int32))}
    keep = {k: v.copy() for k, v in out.items()}

    def call(h=None, null_in=False, null_out=False, omem=abi.MEM_HOST, **kw):
        par = cluster.CubeCorridorIn(batch=4, path_capacity=CAP, mem_in=abi.MEM_HOST, itr_inflate_max=1000, path_xyz=xyz.ctypes.data,
                                     path_len=n.ctypes.data, pop_back=1, seg_capacity=SEG, p_max=6, plane_dtype=abi.F64, resolution=RES,
                                     map_lower=(C.c_double * 3)(*LOWER))
        for k, v in kw.items():
            setattr(par, k, v)
        o = cluster.CubeCorridorOut(omem, 0, *[out[k].ctypes.data for k in KEYS])
        return L.direct_cluster_cube_corridor_batch(gen.h if h is None else h, None if null_in else C.addressof(par),
                                                    None if null_out else C.addressof(o))

    nan, inf = float("nan"), float("inf")
    invalid = [dict(h=C.c_void_p(None)), dict(null_in=True), dict(null_out=True), dict(path_xyz=None), dict(path_len=None), dict(batch=0),
               dict(batch=-1), dict(path_capacity=0), dict(seg_capacity=0), dict(itr_inflate_max=0), dict(p_max=5), dict(mem_in=2),
               dict(omem=2), dict(plane_dtype=2), dict(resolution=0.0), dict(resolution=-0.2), dict(resolution=nan), dict(resolution=inf)]
    for kw in invalid:
        assert call(**kw) == abi.DIRECT_ERR_INVALID, kw
        assert all(out[k].tobytes() == keep[k].tobytes() for k in KEYS), kw
    fresh = cluster.ClusterGenerator(ch.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)   # a handle without a map
    try:
        assert call(h=fresh.h) == abi.DIRECT_ERR_INVALID
    finally:
        fresh.close()
    assert all(out[k].tobytes() == keep[k].tobytes() for k in KEYS)
    assert call() == abi.DIRECT_OK and (out["rtn"] == cluster.CUBE_CORRIDOR_OK).all()
    # NULL outputs are left alone: only the codes
    only = np.full(4, -1, np.int32)
    par = cluster.CubeCorridorIn(batch=4, path_capacity=CAP, mem_in=abi.MEM_HOST, itr_inflate_max=1000, path_xyz=xyz.ctypes.data,
                                 path_len=n.ctypes.data, pop_back=1, seg_capacity=SEG, p_max=6, plane_dtype=abi.F64, resolution=RES,
                                 map_lower=(C.c_double * 3)(*LOWER))
    o = cluster.CubeCorridorOut(abi.MEM_HOST, 0, None, None, None, None, None, None, only.ctypes.data)
    assert L.direct_cluster_cube_corridor_batch(gen.h, C.addressof(par), C.addressof(o)) == abi.DIRECT_OK and not only.any()
    # per-row codes beside good rows
    uturn = next(c for c in ch.named_cases() if c["name"] == "u_turn_no_pop")["paths"][0]
    mixed = [rows[0], uturn, [[24, 0, 0]], rows[1], np.zeros((0, 3), np.int32), uturn]
    mx, mn = ch.pack_paths(mixed, CAP)
    mn[5] = CAP + 1   # an OVERFLOW row of the path stage
    full = gen.cube_corridors(mx, mn, LOWER, RES, pop_back=False, seg_capacity=SEG)
    need = int(full["n_seg"][1])
    cut = gen.cube_corridors(mx, mn, LOWER, RES, pop_back=False, seg_capacity=need - 1)
    B, O, K = cluster.CUBE_CORRIDOR_BAD_PATH, cluster.CUBE_CORRIDOR_OVERFLOW, cluster.CUBE_CORRIDOR_OK
    assert full["rtn"].tolist() == [K, K, B, K, B, B] and need >= 3
    assert cut["rtn"].tolist() == [K if full["n_seg"][0] < need else O, O, B, K if full["n_seg"][3] < need else O, B, B]
    assert np.array_equal(cut["n_seg"], full["n_seg"]) and cut["n_seg"][2] == cut["n_seg"][4] == cut["n_seg"][5] == 0
    for k in ("n_planes", "planes", "seeds", "centers", "cube_idx"):
        assert np.array_equal(cut[k], full[k][:, :need - 1]), k
    alone = gen.cube_corridors(*ch.pack_paths([rows[0]], CAP), LOWER, RES, pop_back=False, seg_capacity=SEG)
    same({k: full[k][:1] for k in KEYS}, alone)


def test_cpp_mirror_against_its_lock_step_walks(gen, rows, tmp_path):
    """8.  polyhedronGenerator::cubeCorridorBatch (direct_amd/host/poly_utils.hpp) gives the corridors of corridorGenerationBatch /
    corridorInsertGenerationBatch on a generator without clustering, bit for bit (tests/cpp/test_cube_corridor_gen.cpp)"""
    fin, exe = str(tmp_path / "in.bin"), str(tmp_path / "gen")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3id3di", *ch.DIMS, RES, *LOWER, len(rows)))
        for p in rows:
            f.write(struct.pack("<i", len(p)))
            f.write(np.ascontiguousarray(p.astype(np.float64) * RES + 0.5 * RES + LOWER, np.float64).tobytes())
        f.write(ch.crafted_map().tobytes())
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests/cpp/test_cube_corridor_gen.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "direct_amd/lib"), "-ldirect_ddp",
                           "-Wl,-rpath," + os.path.join(ROOT, "direct_amd/lib") + ":/opt/rocm/lib"])
    out = subprocess.run([exe, fin], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
