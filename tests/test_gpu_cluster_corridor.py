"""direct_cluster_corridor_batch (include/direct_cluster.h, "cluster corridors"; kernels in direct_amd/csrc/cluster_corridor.h) on
the device, through the C-ABI: against the lock-step walk through the existing calls (tests/cluster_corridor_lib.py), against
oracle.corridor_walk, under other max_batch / row orders / splits, what it does to the handle and what it leaves alone, the per-row
codes, the device-resident chain into direct_ddp_plan_batch, and the C++ mirror.  No row is skipped or filtered: every row that
is not planted to fail must end OK, and every test asserts it."""
import functools

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import cluster_corridor_harness as kh
from tests import cluster_corridor_lib as kl
from tests import corridor_lib as lib
from tests import cube_corridor_harness as ch

pytestmark = pytest.mark.gpu
RES, LOWER = kh.RES, kh.LOWER
CAP, SEG, PMAX, KEYS = kh.CAP, kh.SEG, kh.PMAX, kh.KEYS
OK = cluster.CLUSTER_CORRIDOR_OK
same = functools.partial(lib.same, keys=KEYS)


def make_gen(max_batch=64, capacity=kh.CAPACITY, grid=None):
    g = cluster.ClusterGenerator(ch.DIMS, max_batch=max_batch, cluster_capacity=capacity, candidate_capacity=capacity)
    g.set_map(ch.crafted_map() if grid is None else grid)
    return g


@pytest.fixture(scope="module")
def gen(built):
    g = make_gen()
    yield g
    g.close()


@pytest.fixture(scope="module")
def rows():
    return kh.inside_rows()


def run(gen, rows, **kw):
    xyz, n = ch.pack_paths(rows, CAP)
    kw.setdefault("seg_capacity", SEG)
    kw.setdefault("p_max", PMAX)
    return gen.cluster_corridors(xyz, n, LOWER, RES, **kw)


@pytest.mark.parametrize("itr_cluster_max", [0, 2, 50])
@pytest.mark.parametrize("pop_back", [True, False])
def test_lock_step_parity(gen, rows, pop_back, itr_cluster_max):
    """1.  every output, bit for bit, equals the lock-step walk through polygon_generation + hull_planes: host and device memory,
    both dtypes; at itr_cluster_max = 0 the planes are also those of cube_corridors"""
    import torch
    xyz, n = ch.pack_paths(rows, CAP)
    want = kl.lock_step_walk(gen, rows, LOWER, RES, pop_back, itr_cluster_max, seg_capacity=SEG, p_max=PMAX)
    assert (want["rtn"] == OK).all() and want["n_seg"].max() >= 4
    for dtype in (np.float64, np.float32):
        w = dict(want, **{k: want[k].astype(dtype) for k in ("planes", "seeds", "centers")})
        host = gen.cluster_corridors(xyz, n, LOWER, RES, itr_cluster_max=itr_cluster_max, pop_back=pop_back, seg_capacity=SEG, p_max=PMAX, dtype=dtype)
        assert (host["rtn"] == OK).all()
        same(host, w)
        dev = gen.cluster_corridors(torch.from_numpy(xyz).to("cuda:0"), torch.from_numpy(n).to("cuda:0"), LOWER, RES, itr_cluster_max=itr_cluster_max,
                                    pop_back=pop_back, seg_capacity=SEG, p_max=PMAX, dtype=dtype)
        assert all(v.is_cuda for k, v in dev.items() if k != "stats")
        same(lib.to_host(dev), w)
        for s in (host["stats"], dev["stats"]):
            assert s["rounds"] == want["stats"]["rounds"] and s["due_seeds"] == want["stats"]["due_seeds"] and s["pops"] == want["stats"]["pops"]
            assert 0 < s["unique_seeds"] <= s["due_seeds"]
    if itr_cluster_max == 0:
        cube = gen.cube_corridors(xyz, n, LOWER, RES, pop_back=pop_back, seg_capacity=SEG, p_max=PMAX)
        assert (cube["rtn"] == cluster.CUBE_CORRIDOR_OK).all()
        same(gen.cluster_corridors(xyz, n, LOWER, RES, itr_cluster_max=0, pop_back=pop_back, seg_capacity=SEG, p_max=PMAX), cube)
    print("cluster corridors, %d rows, pop %d, itr %d: %.3f ms, stats %s" % (len(rows), pop_back, itr_cluster_max, gen.last_ms(), host["stats"]))


@pytest.mark.parametrize("itr_cluster_max", [2, 50])
@pytest.mark.parametrize("pop_back", [True, False])
def test_oracle_parity(gen, rows, pop_back, itr_cluster_max):
    """2.  against oracle.corridor_walk row by row: n_seg, n_planes, and planes, centres and seeds as doubles, bit for bit (the
    comparison tests/test_gpu_hull.py makes between device planes and hullapi)"""
    want, _ = kh.oracle_corridors(rows, itr_cluster_max, pop_back)
    got = run(gen, rows, itr_cluster_max=itr_cluster_max, pop_back=pop_back)
    assert (got["rtn"] == OK).all()
    kh.assert_rows_equal_oracle(got, want, rows)


def test_shape_independence(built, gen, rows):
    """3.  max_batch = 2 against 64, a permuted batch and two calls of half the rows give identical bytes; stats for a shared start"""
    xyz, n = ch.pack_paths(rows, CAP)
    one = run(gen, rows)
    assert (one["rtn"] == OK).all()
    small = make_gen(max_batch=2)
    try:
        two = run(small, rows)
        same(two, one)
        assert two["stats"] == one["stats"]
        perm = np.random.default_rng(1).permutation(len(rows))
        p = small.cluster_corridors(xyz[perm], n[perm], LOWER, RES, seg_capacity=SEG, p_max=PMAX)
        same(p, {k: one[k][perm] for k in KEYS})
    finally:
        small.close()
    h = len(rows) // 2
    a = gen.cluster_corridors(xyz[:h], n[:h], LOWER, RES, seg_capacity=SEG, p_max=PMAX)
    b = gen.cluster_corridors(xyz[h:], n[h:], LOWER, RES, seg_capacity=SEG, p_max=PMAX)
    same({k: np.concatenate([a[k], b[k]]) for k in KEYS}, one)
    same(run(gen, rows), one)   # and the used workspace changes nothing
    shared = kh.shared_start_rows()
    got = run(gen, shared)
    s = got["stats"]
    assert (got["rtn"] == OK).all() and s["unique_seeds"] < s["due_seeds"] and s["due_seeds"] >= 6
    alone = [run(gen, [p])["stats"] for p in shared]
    assert s["rounds"] == max(a["rounds"] for a in alone) and s["due_seeds"] == sum(a["due_seeds"] for a in alone)
    assert s["pops"] == sum(a["pops"] for a in alone)


def test_handle_state(gen, rows):
    """4.  the result follows set_map; resident clusters are invalidated; the distance field, the components and an earlier grid-path
    result are unaffected and not stale"""
    grid = ch.crafted_map()
    before = run(gen, rows, itr_cluster_max=2)
    assert (before["rtn"] == OK).all()
    other = ch.random_map(80, 0.08)
    try:   # on the random map no capacity may decide either: one polytope per path point at most, the C++ mirror's 128 planes
        gen.set_map(other)
        got = run(gen, rows, itr_cluster_max=2, seg_capacity=CAP, p_max=128)
        want = kl.lock_step_walk(gen, rows, LOWER, RES, True, 2, seg_capacity=CAP, p_max=128)
    finally:
        gen.set_map(grid)
    assert (got["rtn"] == OK).all()
    same(got, want)
    assert got["planes"][:, :SEG, :PMAX].tobytes() != before["planes"].tobytes()
    same(run(gen, rows, itr_cluster_max=2), before)
    # bystanders
    seeds = np.array([[5, 5, 5], [20, 3, 3]], np.int32)
    starts, goals = np.array([[5, 5, 5], [1, 1, 1]], np.int32), np.array([[22, 18, 10], [20, 12, 5]], np.int32)
    want_path = gen.grid_paths(starts, goals, path_capacity=64, want_dist=True)
    dev_path = gen.grid_paths(starts, goals, path_capacity=64, mem="device")
    keep = {k: v.clone() for k, v in dev_path.items()}
    gen.build_distance_field()
    want_field = gen.distance_field()
    comp = gen.build_free_components(0)
    want_label, want_size = gen.free_components()
    gen.polygon_generation(seeds, 1000, 2, fetch_clusters=False)
    assert (gen.hull_planes(RES, LOWER, batch=2)["rtn"] == cluster.HULL_OK).all()
    fromdev = gen.cluster_corridors(dev_path["path_xyz"], dev_path["path_len"], LOWER, RES, itr_cluster_max=2, seg_capacity=SEG, p_max=PMAX)
    assert (fromdev["rtn"] == OK).all()
    with pytest.raises(solver.DirectError) as e:   # the call used the cluster storage: nothing resident any more
        gen.hull_planes(RES, LOWER, batch=1)
    assert e.value.status == abi.DIRECT_ERR_INVALID
    assert np.array_equal(gen.distance_field(), want_field)   # still valid, still the same
    label, size = gen.free_components()
    assert np.array_equal(label, want_label) and np.array_equal(size, want_size) and comp["components"] >= 1
    for k, v in dev_path.items():
        assert v.cpu().numpy().tobytes() == keep[k].cpu().numpy().tobytes(), k
    again = gen.grid_paths(starts, goals, path_capacity=64, want_dist=True)
    assert (want_path["rtn"] == cluster.GRID_PATH_OK).all() and np.array_equal(again["path_len"], want_path["path_len"])
    assert all(np.array_equal(a, b) for a, b in zip(again["paths"], want_path["paths"]))
    assert np.array_equal(grid, gen.get_map())


def test_per_row_codes(built, gen, rows):
    """5.  NO_POLYTOPE beside OK rows on a handle with cluster_capacity = 200; p_max = 8; a short seg_capacity; bad paths"""
    full = run(gen, rows, pop_back=False)
    assert (full["rtn"] == OK).all()
    tight = make_gen(capacity=200)
    try:
        got = run(tight, rows, pop_back=False)
        want = kl.lock_step_walk(tight, rows, LOWER, RES, False, 50, seg_capacity=SEG, p_max=PMAX)
    finally:
        tight.close()
    same(got, want)
    codes = set(got["rtn"].tolist())
    assert codes == {OK, cluster.CLUSTER_CORRIDOR_NO_POLYTOPE}, codes
    for b in range(len(rows)):
        k = int(got["n_seg"][b])
        assert k <= full["n_seg"][b]
        for key in ("n_planes", "planes", "seeds", "centers"):   # what a stopped row holds is the head of its corridor
            assert np.array_equal(got[key][b, :k], full[key][b, :k]) and not got[key][b, k:].any(), (b, key)
        assert (got["rtn"][b] == OK) == (k == full["n_seg"][b])
    # p_max = 8 against polytopes of up to 16 planes
    few = run(gen, rows, pop_back=False, p_max=8)
    same(few, kl.lock_step_walk(gen, rows, LOWER, RES, False, 50, seg_capacity=SEG, p_max=8))
    stopped = 0
    for b in range(len(rows)):
        wide = [s for s in range(full["n_seg"][b]) if full["n_planes"][b, s] > 8]
        stopped += bool(wide)
        assert few["rtn"][b] == (cluster.CLUSTER_CORRIDOR_TOO_MANY_PLANES if wide else OK)
        assert few["n_seg"][b] == (wide[0] if wide else full["n_seg"][b])
    assert 0 < stopped < len(rows) and full["n_planes"].max() == 16
    # seg_capacity one short of the longest corridor
    need = int(full["n_seg"].max())
    cut = run(gen, rows, pop_back=False, seg_capacity=need - 1)
    over = full["n_seg"] >= need
    assert cut["rtn"].tolist() == [cluster.CLUSTER_CORRIDOR_OVERFLOW if o else OK for o in over] and over.any() and not over.all()
    assert cut["n_seg"].tolist() == [need - 1 if o else int(v) for o, v in zip(over, full["n_seg"])]
    for key in ("n_planes", "planes", "seeds", "centers"):
        assert np.array_equal(cut[key], full[key][:, :need - 1]), key
    # bad paths beside good rows
    B = cluster.CLUSTER_CORRIDOR_BAD_PATH
    mixed = [rows[0], [[24, 0, 0]], rows[1], np.zeros((0, 3), np.int32), rows[2], [[0, -1, 0]]]
    mx, mn = ch.pack_paths(mixed, CAP)
    mn[4] = CAP + 1   # an OVERFLOW row of the path stage
    bad = gen.cluster_corridors(mx, mn, LOWER, RES, pop_back=False, seg_capacity=SEG, p_max=PMAX)
    assert bad["rtn"].tolist() == [OK, B, OK, B, B, B]
    for b in (1, 3, 4, 5):
        assert bad["n_seg"][b] == 0 and not any(bad[k][b].any() for k in ("n_planes", "planes", "seeds", "centers"))
    same({k: bad[k][[0, 2]] for k in KEYS}, {k: full[k][[0, 1]] for k in KEYS})


def test_abi_edges(gen, rows):
    """5b.  every DIRECT_ERR_INVALID case of the header launches nothing (the outputs keep their bytes); NULL outputs are left alone"""
    L = cluster._lib()
    xyz, n = ch.pack_paths(rows[:4], CAP)
    stats = np.full(4, -5, np.int64)

    def entry(h, par, o, stats=stats.ctypes.data):
        return L.direct_cluster_corridor_batch(h, par, o, stats)

    raw = lib.RawCall(gen, entry, cluster.ClusterCorridorIn, cluster.ClusterCorridorOut, KEYS, xyz, n, SEG, PMAX, extras=(stats,),
                      itr_cluster_max=2)
    for kw in lib.INVALID + [dict(itr_cluster_max=-1)]:
        assert raw.call(**kw) == abi.DIRECT_ERR_INVALID, kw
        assert raw.untouched() and (stats == -5).all(), kw
    with lib.handle_without_map() as fresh:
        assert raw.call(h=fresh.h) == abi.DIRECT_ERR_INVALID
    assert raw.untouched()
    assert raw.call(batch=1 << 20, path_capacity=1 << 8) == abi.DIRECT_ERR_UNSUPPORTED
    assert raw.call() == abi.DIRECT_OK and (raw.out["rtn"] == OK).all() and stats[0] > 0
    status, only = raw.only_codes(stats=None)
    assert status == abi.DIRECT_OK and not only.any()


def test_chain_on_the_device_into_the_optimiser(built):
    """6.  grid_paths(mem="device") -> cluster_corridors on device tensors -> direct_ddp_plan_batch with T0 == NULL equals the same
    chain through host arrays to the byte, and every OK row - here every row - is reported with rtn != DIRECT_RTN_INVALID"""
    import torch
    dev = "cuda:0"
    N, P = SEG, PMAX
    gen = make_gen(max_batch=16)
    starts = np.array([[5, 5, 5], [1, 1, 1], [22, 18, 10], [1, 18, 1], [12, 12, 5], [20, 3, 3], [4, 12, 6], [22, 1, 1]], np.int32)
    goals = np.array([[22, 18, 10], [20, 12, 5], [1, 1, 10], [22, 2, 10], [1, 10, 10], [3, 17, 9], [18, 8, 2], [9, 10, 10]], np.int32)
    B = len(starts)
    paths = gen.grid_paths(starts, goals, path_capacity=64, mem="device")
    cor = gen.cluster_corridors(paths["path_xyz"], paths["path_len"], LOWER, RES, itr_cluster_max=50, seg_capacity=N, p_max=P)
    hp = gen.grid_paths(starts, goals, path_capacity=64)
    hx, hn = ch.pack_paths(hp["paths"], 64)
    hcor = gen.cluster_corridors(hx, hn, LOWER, RES, itr_cluster_max=50, seg_capacity=N, p_max=P)
    gen.close()
    assert (hp["rtn"] == cluster.GRID_PATH_OK).all() and (hcor["rtn"] == OK).all()
    same(lib.to_host(cor), hcor)
    x0, xd = lib.chain_ends(paths, torch.arange(B, device=dev))
    hx0, hxd = np.zeros((B, 9)), np.zeros((B, 9))
    hx0[:, :3] = starts * RES + 0.5 * RES + LOWER
    hxd[:, :3] = goals * RES + 0.5 * RES + LOWER
    assert np.array_equal(hx0, x0.cpu().numpy()) and np.array_equal(hxd, xd.cpu().numpy())   # so the host copies are the host chain's
    _, (r0, r1), (_, d1) = lib.plan_chain(cor, x0, xd, N, P)
    print("chain: %d rows, n_seg %s, rtn %s, stats %s" % (B, hcor["n_seg"].tolist(), r1.rtn.tolist(), hcor["stats"]))
    assert (np.asarray(r0.rtn) != abi.RTN_INVALID).all() and (np.asarray(r1.rtn) != abi.RTN_INVALID).all()
    assert (np.asarray(d1.rtn) != abi.RTN_INVALID).all()


@pytest.mark.parametrize("itr_cluster_max", [50])
def test_cpp_mirror_against_its_lock_step_walks(built, rows, tmp_path, itr_cluster_max):
    """7.  polyhedronGenerator::clusterCorridorBatch (direct_amd/host/poly_utils.hpp) gives the corridors of corridorGenerationBatch /
    corridorInsertGenerationBatch from empty corridors, bit for bit (tests/cpp/test_cluster_corridor_gen.cpp)"""
    lib.run_cpp_mirror(tmp_path, "test_cluster_corridor_gen.cpp", rows, args=(itr_cluster_max, kh.CAPACITY))
