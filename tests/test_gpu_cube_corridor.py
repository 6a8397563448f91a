"""direct_cluster_cube_corridor_batch (include/direct_cluster.h, "cube corridors"; kernels in direct_amd/csrc/cube_corridor.h) on
the device, through the C-ABI: against the g++ build of the same arithmetic (tests/cube_corridor_harness.py, itself held against
three independent witnesses by tests/test_cube_corridor_restatement.py), against the path that exists beside it - a lock-step walk
over polygon_generation(seed, itr, 0) + hull_planes() on the same handle -, launch-shape independence, a change of map, what the
call leaves alone, the device-resident chain into direct_ddp_plan_batch, and the edges of the ABI."""
import functools

import numpy as np
import pytest

from direct_amd import abi, cluster
from tests import corridor_lib as lib
from tests import cube_corridor_harness as ch

pytestmark = pytest.mark.gpu
RES, LOWER = ch.RES, ch.LOWER
KEYS = abi.CUBE_CORRIDOR_OUTPUTS
CAP, SEG = 40, 32
same = functools.partial(lib.same, keys=KEYS)


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
    return lib.rows40()


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
        same(lib.to_host(dev), want)
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
    xyz, n = ch.pack_paths(rows, CAP)
    gen.build_distance_field()
    by = lib.Bystanders(gen)
    gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG)
    gen.cube_corridors(by.dev_path["path_xyz"], by.dev_path["path_len"], LOWER, RES, seg_capacity=SEG)
    by.check()


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
    x0, xd = lib.chain_ends(paths, pick)
    h, (_, r1), _ = lib.plan_chain({k: cor[k][pick] for k in ("n_seg", "n_planes", "planes", "seeds")}, x0, xd, N, P)
    print("chain: %d rows, n_seg %s, rtn %s" % (B, h["n_seg"].tolist(), r1.rtn.tolist()))
    assert (h["n_seg"] <= N).all()


def test_abi_edges(gen, rows):
    """7.  every DIRECT_ERR_INVALID case launches nothing (the outputs keep their bytes); OVERFLOW and BAD_PATH rows beside good ones"""
    xyz, n = ch.pack_paths(rows[:4], CAP)
    raw = lib.RawCall(gen, cluster._lib().direct_cluster_cube_corridor_batch, cluster.CubeCorridorIn, cluster.CubeCorridorOut, KEYS, xyz, n,
                      SEG, 6)
    for kw in lib.INVALID:
        assert raw.call(**kw) == abi.DIRECT_ERR_INVALID, kw
        assert raw.untouched(), kw
    with lib.handle_without_map() as fresh:
        assert raw.call(h=fresh.h) == abi.DIRECT_ERR_INVALID
    assert raw.untouched()
    assert raw.call() == abi.DIRECT_OK and (raw.out["rtn"] == cluster.CUBE_CORRIDOR_OK).all()
    # NULL outputs are left alone: only the codes
    status, only = raw.only_codes()
    assert status == abi.DIRECT_OK and not only.any()
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
    lib.run_cpp_mirror(tmp_path, "test_cube_corridor_gen.cpp", rows)
