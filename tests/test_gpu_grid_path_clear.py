"""direct_cluster_grid_path_clear_batch (include/direct_cluster.h, "clearance-aware grid paths"; kernels in
direct_amd/csrc/grid_path_clear.h) on the device, through the C-ABI: neutral parameters against the plain call on the same handle,
the floor against the plain call on the thresholded map, the penalty against the g++ build of the same arithmetic
(tests/grid_path_clear_harness.py, itself checked against an independent Dijkstra by tests/test_grid_path_clear_restatement.py)
bit for bit, launch-shape independence, both memory kinds, OVERFLOW, every refusal, what the call leaves alone, and the
device-resident chain into the optimiser.  16 queries on the 40 x 24 x 12 maps of the harness."""
import ctypes as C

import numpy as np
import pytest

from direct_amd import abi, cluster, devmem, solver
from tests import grid_path_clear_harness as ch

pytestmark = pytest.mark.gpu
KEYS = ("rtn", "path_len", "path_cost", "path_min_d2")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("grid_path_clear_gpu"))


def handle(grid, cap_vox=0, field=True):
    gen = cluster.ClusterGenerator(grid.shape, max_batch=16, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
    if field:
        gen.build_distance_field(cap_vox)
    return gen


@pytest.fixture(scope="module")
def gap(built):
    grid = ch.gap_map()
    d2 = ch.brute_distance_field(grid)
    s, g = ch.queries(grid, d2, 16, seed=3)
    gen = handle(grid)
    assert np.array_equal(gen.distance_field(), d2)
    yield grid, d2, s, g, gen
    gen.close()


@pytest.fixture(scope="module")
def walls(built):
    grid = ch.walls_map()
    d2 = ch.brute_distance_field(grid)
    s, g = ch.queries(grid, d2, 14, seed=1, floor=9)
    gen = handle(grid)
    assert np.array_equal(gen.distance_field(), d2)
    yield grid, d2, s, g, gen
    gen.close()


def same_as_plain(new, old, q):
    assert new["rtn"][q] == old["rtn"][q] and new["path_len"][q] == old["path_len"][q], (q, new["rtn"][q], old["rtn"][q])
    assert bits(new["path_cost"][q]) == bits(old["path_cost"][q]) or (np.isnan(new["path_cost"][q]) and np.isnan(old["path_cost"][q]))
    assert np.array_equal(new["paths"][q], old["paths"][q])
    if old["rtn"][q] in (ch.OK, ch.OVERFLOW, ch.NO_PATH):  # dist where the contract calls it exact; never below the plain call's elsewhere
        near = old["dist"][q] <= (old["path_cost"][q] if old["rtn"][q] != ch.NO_PATH else np.inf)
        assert np.array_equal(bits(new["dist"][q][near]), bits(old["dist"][q][near]))
        assert ((new["dist"][q] <= old["path_cost"][q]) == (old["dist"][q] <= old["path_cost"][q])).all() or old["rtn"][q] == ch.NO_PATH


def same_as_harness(dev, ref, d2, q, qr=None):
    qr = q if qr is None else qr
    assert dev["rtn"][q] == ref["rtn"][qr], (q, dev["rtn"][q], ref["rtn"][qr])
    assert dev["path_len"][q] == ref["path_len"][qr] and dev["path_min_d2"][q] == ref["path_min_d2"][qr]
    assert bits(dev["path_cost"][q]) == bits(ref["path_cost"][qr]) or (np.isnan(dev["path_cost"][q]) and np.isnan(ref["path_cost"][qr]))
    assert np.array_equal(dev["paths"][q], ref["paths"][qr]) and np.array_equal(dev["path_d2"][q], ref["path_d2"][qr])
    if dev.get("dist") is not None and ref["rtn"][qr] in (ch.OK, ch.OVERFLOW, ch.NO_PATH):
        true, got = ref["dist"][qr], dev["dist"][q]
        near = true <= (ref["path_cost"][qr] if ref["rtn"][qr] != ch.NO_PATH else np.inf)
        assert np.array_equal(bits(got[near]), bits(true[near])) and (got[~near] >= true[~near]).all()


def test_neutral_parameters_are_the_plain_call(gap, walls):
    """1.  min_d2 = 0 and no table: grid_paths on the same handle, byte for byte on every output, dist where the contract says
    exact; also with min_d2 = 1 and a table of zeros, and for the codes that compute nothing"""
    for grid, d2, s, g, gen in (gap, walls):
        s = np.concatenate([s[:13], [[-1, 0, 0], [3, 3, 3], [2, 12, 6]]]).astype(np.int32)   # outside, start == goal, an occupied goal
        g = np.concatenate([g[:13], [[1, 1, 1], [3, 3, 3], np.argwhere(grid == 1)[40]]]).astype(np.int32)
        old = gen.grid_paths(s, g, path_capacity=96, want_dist=True)
        for min_d2, pen in ((0, None), (1, np.zeros(7))):
            new = gen.grid_paths_clear(s, g, min_d2, pen, path_capacity=96, want_dist=True)
            for q in range(16):
                same_as_plain(new, old, q)
                assert np.array_equal(new["path_d2"][q], d2[tuple(new["paths"][q].T)])
        assert old["rtn"][13] == ch.BAD_ENDPOINT and old["rtn"][14] == ch.OK and old["path_len"][14] == 1 and old["rtn"][15] == ch.NO_PATH
        assert (new["path_min_d2"][13:] == cluster.DIST_NONE).all() and (old["rtn"][:13] == ch.OK).all()


def test_floor_is_the_plain_call_on_the_thresholded_map(walls):
    """2.  for every floor, grid_paths on a second handle that holds byte | (D2 < min_d2); a goal below the floor is NO_PATH, a
    start below it still works"""
    grid, d2, s, g, gen = walls
    moved = 0
    for min_d2 in (1, 2, 4, 9):
        low = [{1: 6, 2: 5, 4: 5, 9: 4}[min_d2], 10, 5]
        ss = np.concatenate([s, [[2, 12, 6], low]]).astype(np.int32)
        gg = np.concatenate([g, [low, [38, 12, 6]]]).astype(np.int32)
        other = handle((grid | (d2 < min_d2)).astype(np.uint8), field=False)
        old = other.grid_paths(ss, gg, want_dist=True)
        other.close()
        new = gen.grid_paths_clear(ss, gg, min_d2, want_dist=True)
        for q in range(16):
            same_as_plain(new, old, q)
        assert (new["rtn"][:14] == ch.OK).all() and new["rtn"][14] == ch.NO_PATH and new["rtn"][15] == ch.OK
        assert (new["path_min_d2"][:14] >= min_d2).all() and new["path_min_d2"][14] == cluster.DIST_NONE
        plain = gen.grid_paths(ss, gg)
        moved += any(not np.array_equal(new["paths"][q], plain["paths"][q]) for q in range(14))
    assert moved >= 3  # the floors 2, 4 and 9 each close a gap the plain paths use


@pytest.mark.parametrize("min_d2,table", [(0, (0.3, 4.0)), (0, (1.0, 4.0)), (2, (0.3, 4.0))], ids=["w0.3_r4", "w1.0_r4", "floor2_w0.3_r4"])
def test_penalty_against_the_harness(gap, harness, min_d2, table):
    """3.  path_xyz, path_len, path_cost, rtn, path_d2, path_min_d2 bit for bit, dist where D <= path_cost"""
    grid, d2, s, g, gen = gap
    pen = cluster.clearance_penalty_table(*table)
    ref = ch.run(harness, grid, d2, s, g, min_d2, pen, sides=("full",))["full"]
    dev = gen.grid_paths_clear(s, g, min_d2, pen, want_dist=True)
    print("device: %.3f ms, rounds %s, tile visits %s" % (gen.last_ms(), dev["stats"][:, 0].tolist(), dev["stats"][:, 1].tolist()))
    for q in range(16):
        same_as_harness(dev, ref, d2, q)
    plain = gen.grid_paths(s, g)
    assert (dev["rtn"] == ch.OK).all() and sum(not np.array_equal(dev["paths"][q], plain["paths"][q]) for q in range(16)) >= 8
    assert np.isposinf(dev["dist"][:, grid.ravel() != 0]).all()


def pack(r, order=None):
    n = len(r["paths"])
    order = list(range(n) if order is None else order)
    xyz, pd2 = np.zeros((n, 4096, 3), np.int32), np.zeros((n, 4096), np.int32)
    for i, q in enumerate(order):
        xyz[i, :len(r["paths"][q])] = r["paths"][q]
        pd2[i, :len(r["path_d2"][q])] = r["path_d2"][q]
    return xyz.tobytes() + pd2.tobytes() + b"".join(r[k][order].tobytes() for k in KEYS)


def test_launch_shape_independence(gap):
    """4.  one call of 16, two of 8 and a permuted batch give identical bytes; so does a second call on the used workspace"""
    grid, d2, s, g, gen = gap
    pen = cluster.clearance_penalty_table(0.3, 4.0)
    one = gen.grid_paths_clear(s, g, 2, pen)
    assert pack(one) == pack(gen.grid_paths_clear(s, g, 2, pen))
    h0, h1 = gen.grid_paths_clear(s[:8], g[:8], 2, pen), gen.grid_paths_clear(s[8:], g[8:], 2, pen)
    halves = dict(paths=h0["paths"] + h1["paths"], path_d2=h0["path_d2"] + h1["path_d2"], **{k: np.concatenate([h0[k], h1[k]]) for k in KEYS})
    assert pack(one) == pack(halves)
    perm = np.random.default_rng(1).permutation(16)
    assert pack(one, perm) == pack(gen.grid_paths_clear(s[perm], g[perm], 2, pen))
    a, c = gen.grid_paths_clear(s[:8], g[:8], 2, pen, want_dist=True), gen.grid_paths_clear(s[:8][::-1], g[:8][::-1], 2, pen, want_dist=True)
    for q in range(8):
        near = a["dist"][q] <= a["path_cost"][q]
        assert np.array_equal(bits(a["dist"][q][near]), bits(c["dist"][7 - q][near]))
        assert ((c["dist"][7 - q] <= a["path_cost"][q]) == near).all()


def test_memory_kinds_and_overflow(gap, harness):
    """5.  outputs in device memory equal outputs in host memory; a path_capacity one too small reports OVERFLOW with the needed
    path_len and the whole path's path_min_d2, in both kinds; NULL outputs are left alone"""
    grid, d2, s, g, gen = gap
    pen = cluster.clearance_penalty_table(1.0, 4.0)
    host = gen.grid_paths_clear(s, g, 0, pen, path_capacity=64)
    dev = gen.grid_paths_clear(s, g, 0, pen, path_capacity=64, mem="device")
    for k in KEYS:
        assert dev[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    for q in range(16):
        n = host["path_len"][q]
        assert np.array_equal(dev["path_xyz"][q, :n].cpu().numpy(), host["paths"][q])
        assert np.array_equal(dev["path_d2"][q, :n].cpu().numpy(), host["path_d2"][q])
    q = int(np.argmax(host["path_len"]))
    cap = int(host["path_len"][q]) - 1
    small = gen.grid_paths_clear(s[q:q + 1], g[q:q + 1], 0, pen, path_capacity=cap)
    small_dev = gen.grid_paths_clear(s[q:q + 1], g[q:q + 1], 0, pen, path_capacity=cap, mem="device")
    for r in (small, {k: v.cpu().numpy() for k, v in small_dev.items()}):
        assert r["rtn"][0] == ch.OVERFLOW and r["path_len"][0] == cap + 1 and r["path_min_d2"][0] == host["path_min_d2"][q]
        assert bits(r["path_cost"][0]) == bits(host["path_cost"][q])
    assert np.array_equal(small["paths"][0], host["paths"][q][:cap]) and np.array_equal(small["path_d2"][0], host["path_d2"][q][:cap])
    assert np.array_equal(small_dev["path_xyz"][0].cpu().numpy(), host["paths"][q][:cap])
    assert host["path_min_d2"][q] == d2[tuple(host["paths"][q][1:].T)].min()
    only = np.full(16, -1, np.int32)
    par = abi.GridPathClearIn(batch=16, path_capacity=64, mem=abi.MEM_HOST, starts=s.ctypes.data, goals=g.ctypes.data, n_penalty=len(pen),
                              penalty=pen.ctypes.data)
    out = abi.GridPathClearOut(path_min_d2=only.ctypes.data)
    assert cluster._lib().direct_cluster_grid_path_clear_batch(gen.h, C.addressof(par), C.addressof(out)) == abi.DIRECT_OK
    assert np.array_equal(only, host["path_min_d2"])


def refused(call):
    with pytest.raises(solver.DirectError) as e:
        call()
    return e.value.status == abi.DIRECT_ERR_INVALID


def test_refusals(built):
    """6.  all DIRECT_ERR_INVALID: a field stale after set_map, no field ever built, a capped field with min_d2 or n_penalty above
    cap2, and a NaN, a negative and an infinite table entry"""
    grid = ch.gap_map()
    s, g = np.array([[1, 1, 1]], np.int32), np.array([[38, 20, 10]], np.int32)
    gen = handle(grid, field=False)
    assert refused(lambda: gen.grid_paths_clear(s, g))                       # no field ever built
    gen.build_distance_field(3)                                                # cap2 = 9
    assert gen.grid_paths_clear(s, g, 9, np.zeros(9))["rtn"][0] in (ch.OK, ch.NO_PATH)
    assert refused(lambda: gen.grid_paths_clear(s, g, 10))                   # min_d2 > cap2
    assert refused(lambda: gen.grid_paths_clear(s, g, 0, np.zeros(10)))      # n_penalty > cap2
    for bad in (np.nan, -1.0, np.inf):
        t = np.zeros(9)
        t[4] = bad
        assert refused(lambda: gen.grid_paths_clear(s, g, 0, t)), bad
    gen.set_map(grid)
    assert refused(lambda: gen.grid_paths_clear(s, g))                       # stale after set_map: never rebuilt silently
    gen.build_distance_field()
    assert gen.grid_paths_clear(s, g, 10, np.zeros(10))["rtn"][0] in (ch.OK, ch.NO_PATH)   # an uncapped field refuses neither
    assert gen.grid_paths(s, g)["rtn"][0] == ch.OK
    gen.close()


def test_leaves_the_rest_of_the_handle_alone(built):
    """7.  resident clusters, the distance field and a following plain grid_paths call are unaffected; the call may also come
    first and allocate the shared workspace"""
    from direct_amd import problems
    RES, LOWER = 0.2, np.array([-12.0, -12.0, 0.0])
    grid, seeds = problems.make_voxel_map()
    seeds = seeds[:8]
    free = np.argwhere(grid == 0)
    rng = np.random.default_rng(2)
    s, g = free[rng.integers(len(free), size=8)].astype(np.int32), free[rng.integers(len(free), size=8)].astype(np.int32)
    first = cluster.ClusterGenerator(grid.shape, max_batch=8, cluster_capacity=50000, candidate_capacity=10000)
    first.set_map(grid)
    want_plain = first.grid_paths(s, g)
    first.polygon_generation(seeds, fetch_clusters=False)
    want_hull = first.hull_planes(RES, LOWER, batch=len(seeds))
    first.close()
    gen = cluster.ClusterGenerator(grid.shape, max_batch=8, cluster_capacity=50000, candidate_capacity=10000)
    gen.set_map(grid)
    gen.build_distance_field()
    field = gen.distance_field()
    gen.polygon_generation(seeds, fetch_clusters=False)
    got = gen.grid_paths_clear(s, g, 0, cluster.clearance_penalty_table(0.5, 5.0))   # the first path call of this handle
    got_hull = gen.hull_planes(RES, LOWER, batch=len(seeds))
    plain = gen.grid_paths(s, g)
    assert np.array_equal(gen.distance_field(), field) and np.array_equal(gen.get_map(), grid)
    gen.close()
    assert (got["rtn"] == ch.OK).sum() >= 4 and (want_hull["rtn"] == cluster.HULL_OK).all()
    for k in ("rtn", "n_planes", "n_vertices", "degenerate", "center"):
        assert np.array_equal(want_hull[k], got_hull[k]), k
    for b in range(len(seeds)):
        for k in ("planes", "plane_int", "vertices"):
            assert np.array_equal(want_hull[k][b], got_hull[k][b]), (k, b)
    for k in ("rtn", "path_len"):
        assert np.array_equal(plain[k], want_plain[k])
    assert np.array_equal(bits(plain["path_cost"]), bits(want_plain["path_cost"]))
    assert all(np.array_equal(a, b) for a, b in zip(plain["paths"], want_plain["paths"]))


def test_chain_on_the_device_into_the_optimiser(built):
    """8.  set_map_from_cloud -> build_distance_field -> grid_paths_clear(mem="device") -> cube_corridors -> direct_ddp_plan_batch
    runs device-resident and gives the bytes of the same arrays passed through host memory.  The plumbing and the layout are
    under test, not the solver: no return code is asked for."""
    import torch
    RES, LOWER = 0.25, np.array([-5.0, -3.0, 0.0])
    dev = "cuda:0"
    N, P = 12, 6
    cloud = (np.argwhere(ch.gap_map() == 1) * RES + 0.5 * RES + LOWER).astype(np.float32)
    gen = cluster.ClusterGenerator(ch.gap_map().shape, max_batch=16, cluster_capacity=64, candidate_capacity=64)
    gen.set_map_from_cloud(torch.from_numpy(cloud).to(dev), LOWER, RES, cloud_margin=0.0)
    grid = gen.get_map()
    gen.build_distance_field()
    s, g = ch.queries(grid, gen.distance_field(), 16, seed=3)
    pen = cluster.clearance_penalty_table(1.0, 4.0)
    paths = gen.grid_paths_clear(s, g, 2, pen, path_capacity=64, mem="device")
    host_paths = gen.grid_paths_clear(s, g, 2, pen, path_capacity=64)
    cor = gen.cube_corridors(paths["path_xyz"], paths["path_len"], LOWER, RES, seg_capacity=N, p_max=P)
    xyz = np.zeros((16, 64, 3), np.int32)
    for q in range(16):
        xyz[q, :len(host_paths["paths"][q])] = host_paths["paths"][q]
    host_cor = gen.cube_corridors(xyz, host_paths["path_len"], LOWER, RES, seg_capacity=N, p_max=P)
    gen.close()
    for k in abi.CUBE_CORRIDOR_OUTPUTS:
        assert cor[k].cpu().numpy().tobytes() == host_cor[k].tobytes(), k
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
    sol = solver.DdpSolver(B, N, P, np.float64, device=0)
    o0, o1 = devmem.DeviceResult(B, N, np.float64, dev), devmem.DeviceResult(B, N, np.float64, dev)
    torch.cuda.synchronize()
    sol.plan_device(p0, p1, cin, o0.cout, o1.cout)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in t.items()}
    hb = abi.HostBatch(h["n_seg"], h["x0"], h["xd"], np.zeros((B, N)), h["n_planes"], h["planes"], seeds=h["seeds"]).without_T0()
    r0, r1 = sol.plan(p0, p1, hb)
    sol.close()
    d0, d1 = o0.to_host(), o1.to_host()
    print("chain: %d rows, n_seg %s, rtn %s" % (B, h["n_seg"].tolist(), r1.rtn.tolist()))
    for dv, hv in ((d0, r0), (d1, r1)):
        for k in ("rtn", "iter_used", "fwd_passes", "cost", "T", "bez", "poly"):
            assert np.asarray(getattr(dv, k)).tobytes() == np.asarray(getattr(hv, k)).tobytes(), k
    assert (h["n_seg"] <= N).all()
