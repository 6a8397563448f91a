"""direct_cluster_grid_path_fan_batch (include/direct_cluster.h, "shared-start grid paths"; kernels in direct_amd/csrc/grid_path_fan.h)
on the device, through the C-ABI, on a handle with max_batch = 4 and maps of 40 x 24 x 12 and 20 x 17 x 11: every goal of a fan
against the PAIRWISE call on the same handle (grid_paths in neutral mode, grid_paths_clear otherwise, four pairs per call) and against
the g++ build of the same arithmetic (tests/grid_path_fan_harness.py, itself held against an independent Dijkstra by
tests/test_grid_path_fan_restatement.py) bit for bit; grouping independence, both memory kinds, dist, the named cases, the refusals
that need a handle, what the call leaves alone, and the device-resident chain into the optimiser."""
import numpy as np
import pytest

from direct_amd import abi, cluster, devmem, solver
from tests import grid_path_clear_harness as ch
from tests import grid_path_fan_harness as fh
from tests import grid_path_harness as gh

pytestmark = pytest.mark.gpu
MAX_BATCH = 4


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return fh.build(tmp_path_factory.mktemp("grid_path_fan_gpu"))


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return gh.build(tmp_path_factory.mktemp("fan_gpu_ref_plain")), ch.build(tmp_path_factory.mktemp("fan_gpu_ref_clear"))


def handle(grid, field=True, cap_vox=0):
    gen = cluster.ClusterGenerator(grid.shape, max_batch=MAX_BATCH, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
    if field:
        gen.build_distance_field(cap_vox)
    return gen


@pytest.fixture(scope="module")
def walls(built):
    grid = ch.walls_map()
    d2 = ch.brute_distance_field(grid)
    gen = handle(grid)
    assert np.array_equal(gen.distance_field(), d2)
    yield grid, d2, gen
    gen.close()


@pytest.fixture(scope="module")
def gap(built):
    grid = ch.gap_map()
    d2 = ch.brute_distance_field(grid)
    gen = handle(grid)
    yield grid, d2, gen
    gen.close()


@pytest.fixture(scope="module")
def small(built):
    grid = gh.random_map((20, 17, 11), 21, 0.25)
    d2 = ch.brute_distance_field(grid)
    gen = handle(grid)
    yield grid, d2, gen
    gen.close()


def draw(grid, n_src, per, seed, ok=None):
    """n_src sources among the voxels of `ok` (default: free) and per goals each: mostly voxels of `ok`, every fifth any voxel of the
    map (occupied ones included), the last two of each source the source itself and a voxel outside the map"""
    rng = np.random.default_rng(seed)
    good = np.argwhere((grid == 0) if ok is None else ok)
    every = np.argwhere(np.ones(grid.shape, bool))
    sources = good[rng.choice(len(good), n_src, replace=False)].astype(np.int32)
    goals = good[rng.integers(len(good), size=n_src * per)].astype(np.int32)
    goals[::5] = every[rng.integers(len(every), size=len(goals[::5]))]
    gs = np.repeat(np.arange(n_src, dtype=np.int32), per)
    for s in range(n_src):
        goals[(s + 1) * per - 2] = sources[s]
        goals[(s + 1) * per - 1] = [grid.shape[0], 0, 0]
    perm = rng.permutation(len(goals))   # the goals of a source are NOT contiguous in the caller's list
    return sources, goals[perm], gs[perm]


def pairwise(gen, sources, goals, gs, cap, min_d2=0, penalty=None):
    """the pairwise call on the same handle, pair by pair in chunks of max_batch -> the host-layout dict per goal"""
    clear = fh.is_clear(min_d2, penalty)
    starts = sources[gs]
    out = dict(paths=[], path_d2=[], rtn=[], path_len=[], path_cost=[], path_min_d2=[])
    for a in range(0, len(goals), MAX_BATCH):
        s, g = starts[a:a + MAX_BATCH], goals[a:a + MAX_BATCH]
        r = gen.grid_paths_clear(s, g, min_d2, penalty, path_capacity=cap) if clear else gen.grid_paths(s, g, path_capacity=cap)
        out["paths"] += r["paths"]
        out["path_d2"] += r.get("path_d2", [None] * len(g))
        for k in ("rtn", "path_len", "path_cost"):
            out[k].append(r[k])
        out["path_min_d2"].append(r["path_min_d2"] if clear else np.zeros(len(g), np.int32))
    for k in ("rtn", "path_len", "path_cost", "path_min_d2"):
        out[k] = np.concatenate(out[k])
    return out


def pack(r, clear, order=None, cap=96):
    """every per-goal byte of a host-layout result, the goals in `order`"""
    order = list(range(len(r["paths"])) if order is None else order)
    n = len(order)
    xyz, pd2 = np.zeros((n, cap, 3), np.int32), np.zeros((n, cap), np.int32)
    for i, q in enumerate(order):
        xyz[i, :len(r["paths"][q])] = r["paths"][q]
        if clear:
            pd2[i, :len(r["path_d2"][q])] = r["path_d2"][q]
    cost = np.ascontiguousarray(r["path_cost"][order])
    cost[np.isnan(cost)] = np.nan   # one NaN
    keys = ("rtn", "path_len") + (("path_min_d2",) if clear else ())
    return xyz.tobytes() + pd2.tobytes() + cost.tobytes() + b"".join(np.ascontiguousarray(r[k][order]).tobytes() for k in keys)


def test_neutral_fan_is_the_pairwise_call(walls, small):
    """1.  3 sources x 100 goals - n_goal is 75 times max_batch and beyond one wave's 64 - in neutral mode: every per-goal output
    equals grid_paths on the same handle, called pair by pair in chunks of 4.  THE test that pins the feature's claim."""
    for grid, d2, gen in (walls, small):
        sources, goals, gs = draw(grid, 3, 100, seed=5)
        fan = gen.grid_paths_fan(sources, goals, gs, path_capacity=96)
        ms, stats = gen.last_ms(), fan["stats"]
        ref = pairwise(gen, sources, goals, gs, 96)
        print("fan %s: %.3f ms, rounds %s, tile visits %s, codes %s" % (grid.shape, ms, stats[:, 0].tolist(), stats[:, 1].tolist(),
                                                                         np.bincount(fan["rtn"], minlength=5).tolist()))
        assert "path_d2" not in fan and "path_min_d2" not in fan
        fh.same_per_goal(fan, ref, False, str(grid.shape))
        assert pack(fan, False) == pack(ref, False)
        assert (fan["rtn"] == fh.OK).sum() >= 150 and (fan["rtn"] == fh.NO_PATH).sum() >= 3 and (fan["rtn"] == fh.BAD_ENDPOINT).sum() == 3
        assert min(fan["path_len"][fan["rtn"] == fh.OK]) == 1


@pytest.mark.parametrize("case", ["walls_floor4", "walls_floor9", "gap_table", "gap_floor2_table", "small_floor2", "small_table"])
def test_clear_fan_is_the_pairwise_clear_call_and_the_harness(walls, gap, small, harness, case):
    """2.  floor and table cases: equal to grid_paths_clear pairwise and to the CPU harness, bit for bit"""
    grid, d2, gen = dict(walls=walls, gap=gap, small=small)[case.split("_")[0]]
    kw = dict(walls_floor4=dict(min_d2=4), walls_floor9=dict(min_d2=9), gap_table=dict(penalty=cluster.clearance_penalty_table(0.3, 4.0)),
              gap_floor2_table=dict(min_d2=2, penalty=cluster.clearance_penalty_table(1.0, 4.0)), small_floor2=dict(min_d2=2),
              small_table=dict(min_d2=1, penalty=ch.soft_table(0.3, 2.0)))[case]
    ok = (grid == 0) & (d2 >= kw.get("min_d2", 0))
    sources, goals, gs = draw(grid, 3, 24, seed=9, ok=ok)
    fan = gen.grid_paths_fan(sources, goals, gs, path_capacity=96, **kw)
    ref = pairwise(gen, sources, goals, gs, 96, **kw)
    cpu = fh.run(harness, grid, sources, goals, gs, d2, path_capacity=96, fields=False, **kw)
    fh.same_per_goal(fan, ref, True, case + " pairwise")
    fh.same_per_goal(fan, cpu, True, case + " harness")
    assert pack(fan, True) == pack(ref, True) == pack(cpu, True)
    assert (fan["rtn"] == fh.OK).sum() >= (3 if case.startswith("small") else 40)
    for j in np.flatnonzero(fan["rtn"] == fh.OK):
        assert np.array_equal(fan["path_d2"][j], d2[tuple(fan["paths"][j].T)])


@pytest.mark.parametrize("mode", ["neutral", "clear"])
def test_grouping_independence(walls, mode):
    """3.  one call, the goals split over three calls, a permuted goal list, and the sources permuted with goal_src remapped give
    identical bytes per goal; so does a second call on the used workspace"""
    grid, d2, gen = walls
    kw = dict(neutral={}, clear=dict(min_d2=2, penalty=cluster.clearance_penalty_table(0.3, 4.0)))[mode]
    clear = mode == "clear"
    sources, goals, gs = draw(grid, 3, 30, seed=11)
    one = gen.grid_paths_fan(sources, goals, gs, path_capacity=96, **kw)
    want = pack(one, clear)
    assert want == pack(gen.grid_paths_fan(sources, goals, gs, path_capacity=96, **kw), clear)
    parts = [gen.grid_paths_fan(sources, goals[a:b], gs[a:b], path_capacity=96, **kw) for a, b in ((0, 7), (7, 70), (70, 90))]
    split = dict(paths=sum((p["paths"] for p in parts), []), path_d2=sum((p.get("path_d2", []) for p in parts), []))
    for k in ("rtn", "path_len", "path_cost") + (("path_min_d2",) if clear else ()):
        split[k] = np.concatenate([p[k] for p in parts])
    assert want == pack(split, clear)
    perm = np.random.default_rng(2).permutation(len(goals))
    assert pack(one, clear, perm) == pack(gen.grid_paths_fan(sources, goals[perm], gs[perm], path_capacity=96, **kw), clear)
    sp = np.array([2, 0, 1])                      # new source i is old source sp[i]
    remap = np.argsort(sp).astype(np.int32)      # old index -> new index
    assert want == pack(gen.grid_paths_fan(sources[sp], goals, remap[gs], path_capacity=96, **kw), clear)
    # a source alone (goal_src NULL) gives its goals the same bytes
    mine = np.flatnonzero(gs == 1)
    assert pack(one, clear, mine) == pack(gen.grid_paths_fan(sources[1:2], goals[mine], None, path_capacity=96, **kw), clear)


@pytest.mark.parametrize("mode", ["neutral", "clear"])
def test_memory_kinds_and_dist(walls, refs, mode):
    """4.  outputs in device memory equal outputs in host memory, and dist is exact, against the independent Dijkstra, wherever the
    true distance is <= the worst eligible goal's cost, and never below the true distance"""
    grid, d2, gen = walls
    kw = dict(neutral={}, clear=dict(min_d2=2, penalty=cluster.clearance_penalty_table(0.3, 4.0)))[mode]
    clear = mode == "clear"
    sources, goals, gs = draw(grid, 3, 20, seed=13)
    near = np.abs(goals - sources[gs]).max(axis=1) <= 12     # goals close to their sources: the bound prunes
    near |= (goals == [grid.shape[0], 0, 0]).all(axis=1)
    goals, gs = goals[near], gs[near]
    host = gen.grid_paths_fan(sources, goals, gs, path_capacity=64, want_dist=True, **kw)
    dev = gen.grid_paths_fan(sources, goals, gs, path_capacity=64, mem="device", **kw)
    for k in ("rtn", "path_len", "path_cost") + (("path_min_d2",) if clear else ()):
        a, b = dev[k].cpu().numpy(), host[k]
        assert a.tobytes() == b.tobytes() or (k == "path_cost" and np.array_equal(bits(a)[~np.isnan(b)], bits(b)[~np.isnan(b)])), k
    assert ("path_d2" in dev) == clear
    for j in range(len(goals)):
        n = min(int(host["path_len"][j]), 64)
        assert np.array_equal(dev["path_xyz"][j, :n].cpu().numpy(), host["paths"][j])
        if clear:
            assert np.array_equal(dev["path_d2"][j, :n].cpu().numpy(), host["path_d2"][j])
    ref = fh.pairwise(refs[0], refs[1], grid, sources, goals, gs, d2, path_capacity=64, **kw)
    fh.same_per_goal(host, ref, clear, "dijkstra")
    worst = fh.check_dist(host, ref, grid, sources, goals, gs, d2, kw.get("min_d2", 0), clear, mode)
    pruned = sum(int((np.isinf(host["dist"][s]) & np.isfinite(ref["dist"][int(np.flatnonzero(gs == s)[0])])).sum()) for s in range(3))
    print("worst eligible costs %s, voxels left unrelaxed %d" % (worst, pruned))
    assert pruned > 0 or clear   # (under a floor an eligible goal may be cut off, which rightly switches pruning off)
    assert np.isposinf(host["dist"][:, grid.ravel() != 0]).all()


@pytest.mark.parametrize("mode", ["neutral", "clear"])
def test_named_cases(walls, refs, mode):
    """5.  goal == source on an occupied voxel; an occupied goal beside reachable ones with pruning still on; a goal outside the map;
    a source outside the map; a source with no goals; duplicate goals; two sources on one voxel; a capacity one too small;
    max_rounds = 1"""
    grid, d2, gen = walls
    kw = dict(neutral={}, clear=dict(min_d2=2, penalty=ch.soft_table(0.3, 3.0)))[mode]
    clear = mode == "clear"
    floor = kw.get("min_d2", 0)

    def both(sources, goals, gs, cap, **more):
        got = gen.grid_paths_fan(sources, goals, gs, path_capacity=cap, want_dist=True, **kw, **more)
        if not more:
            ref = fh.pairwise(refs[0], refs[1], grid, sources, goals, gs, d2, path_capacity=cap, **kw)
            fh.same_per_goal(got, ref, clear, "named")
            return got, ref, fh.check_dist(got, ref, grid, sources, goals, gs, d2, floor, clear, "named")
        return got

    # goal == source on an occupied voxel
    got, _, _ = both(np.array([[6, 0, 5]], np.int32), np.array([[6, 0, 5], [3, 8, 5]], np.int32), None, 64)
    assert grid[6, 0, 5] == 1 and got["rtn"][0] == fh.OK and got["path_len"][0] == 1 and got["path_cost"][0] == 0.0
    assert got["rtn"][1] == (fh.NO_PATH if clear else fh.OK)
    # an occupied goal beside reachable ones: pruning stays on
    sources = np.array([[2, 10, 5]], np.int32)
    goals = np.array([[4, 12, 6], [6, 1, 5], [1, 6, 3], [0, 0, 0]], np.int32)
    got, ref, worst = both(sources, goals, None, 64)
    assert list(got["rtn"]) == [fh.OK, fh.NO_PATH, fh.OK, fh.NO_PATH] and worst[0] == max(got["path_cost"][0], got["path_cost"][2])
    pruned = np.isinf(got["dist"][0]) & np.isfinite(ref["dist"][0])
    assert pruned.sum() > grid.size // 4 and (ref["dist"][0][pruned] > worst[0]).all()
    # bad endpoints, a source without goals, duplicates, twin sources
    sources = np.array([[2, 10, 5], [40, 0, 0], [30, 3, 3], [2, 10, 5]], np.int32)
    goals = np.array([[10, 12, 6], [3, 24, 0], [10, 12, 6], [1, 1, 1], [2, 2, 2], [10, 12, 6], [38, 20, 9]], np.int32)
    gs = np.array([0, 0, 0, 1, 1, 3, 3], np.int32)
    got, _, _ = both(sources, goals, gs, 128)
    assert list(got["rtn"]) == [fh.OK, fh.BAD_ENDPOINT, fh.OK, fh.BAD_ENDPOINT, fh.BAD_ENDPOINT, fh.OK, fh.OK]
    assert np.array_equal(got["paths"][0], got["paths"][2]) and np.array_equal(got["paths"][0], got["paths"][5])
    assert got["stats"][1].tolist() == [0, 0] and got["stats"][2].tolist() == [1, 1]
    assert np.isinf(got["dist"][2]).sum() == grid.size - 1 and np.isinf(got["dist"][1]).all()
    # a capacity one too small
    sources, goals = np.array([[2, 10, 5]], np.int32), np.array([[25, 5, 5], [4, 10, 5]], np.int32)
    full, _, _ = both(sources, goals, None, 256)
    need = int(full["path_len"][0])
    got, _, _ = both(sources, goals, None, need - 1)
    assert list(got["rtn"]) == [fh.OVERFLOW, fh.OK] and got["path_len"][0] == need and got["path_cost"][0] == full["path_cost"][0]
    assert np.array_equal(got["paths"][0], full["paths"][0][:need - 1])
    if clear:
        assert got["path_min_d2"][0] == full["path_min_d2"][0] == d2[tuple(full["paths"][0][1:].T)].min()
    # max_rounds = 1: exactly the sources still active
    sources = np.array([[2, 10, 5], [30, 3, 3], [38, 20, 9]], np.int32)
    goals = np.array([[38, 20, 9], [2, 10, 5], [30, 3, 3], [3, 10, 5], [38, 20, 9]], np.int32)
    got = both(sources, goals, np.array([0, 0, 1, 0, 2], np.int32), 256, max_rounds=1)
    assert list(got["rtn"]) == [fh.ROUND_LIMIT, fh.ROUND_LIMIT, fh.OK, fh.ROUND_LIMIT, fh.OK]
    assert (got["path_len"][[0, 1, 3]] == 0).all() and np.isnan(got["path_cost"][[0, 1, 3]]).all() and got["path_len"][2] == 1


def refused(call, word):
    with pytest.raises(solver.DirectError) as e:
        call()
    return e.value.status == abi.DIRECT_ERR_INVALID and word in str(e.value)


def test_refusals_that_need_a_handle(built):
    """6.  no map; more sources than max_batch; in clear mode no field, a stale field and the cap rule; neutral mode with a stale or
    missing field works"""
    grid = ch.gap_map()
    s, g = np.array([[1, 1, 1]], np.int32), np.array([[38, 20, 10], [5, 5, 5]], np.int32)
    gen = cluster.ClusterGenerator(grid.shape, max_batch=MAX_BATCH, cluster_capacity=64, candidate_capacity=64)
    assert refused(lambda: gen.grid_paths_fan(s, g), "no map")
    gen.set_map(grid)
    assert refused(lambda: gen.grid_paths_fan(np.zeros((MAX_BATCH + 1, 3), np.int32), g, np.zeros(2, np.int32)), "max_batch")
    assert refused(lambda: gen.grid_paths_fan(s, g, min_d2=2), "distance field")                    # no field ever built
    want = gen.grid_paths_fan(s, g)                                                                # neutral: no field needed
    assert (want["rtn"] == fh.OK).all()
    gen.build_distance_field(3)                                                                    # cap2 = 9
    assert (gen.grid_paths_fan(s, g, min_d2=9, penalty=np.zeros(9))["rtn"] <= fh.NO_PATH).all()
    assert refused(lambda: gen.grid_paths_fan(s, g, min_d2=10), "cap2")
    assert refused(lambda: gen.grid_paths_fan(s, g, penalty=np.zeros(10)), "cap2")
    gen.set_map(grid)
    assert refused(lambda: gen.grid_paths_fan(s, g, min_d2=2), "distance field")                    # stale after set_map
    again = gen.grid_paths_fan(s, g, min_d2=1)                                                     # neutral with a stale field
    assert pack(again, False, cap=512) == pack(want, False, cap=512)
    gen.build_distance_field()
    assert (gen.grid_paths_fan(s, g, min_d2=10, penalty=np.zeros(10))["rtn"] <= fh.NO_PATH).all()   # an uncapped field refuses neither
    gen.close()


def test_leaves_the_rest_of_the_handle_alone(built):
    """7.  resident clusters, the distance field and a cube-corridor result are untouched; following grid_paths / grid_paths_clear
    calls give the bytes they gave before; a fan call after a set_map sees the new map; the fan may be the handle's first path call"""
    import torch
    from direct_amd import problems
    RES, LOWER = 0.2, np.array([-12.0, -12.0, 0.0])
    grid, seeds = problems.make_voxel_map()
    seeds = seeds[:4]
    free = np.argwhere(grid == 0)
    rng = np.random.default_rng(2)
    s, g = free[rng.integers(len(free), size=4)].astype(np.int32), free[rng.integers(len(free), size=4)].astype(np.int32)
    pen = cluster.clearance_penalty_table(0.5, 5.0)
    first = cluster.ClusterGenerator(grid.shape, max_batch=MAX_BATCH, cluster_capacity=50000, candidate_capacity=10000)
    first.set_map(grid)
    first.build_distance_field()
    want_plain, want_clear = first.grid_paths(s, g, path_capacity=512), first.grid_paths_clear(s, g, 0, pen, path_capacity=512)
    first.polygon_generation(seeds, fetch_clusters=False)
    want_hull = first.hull_planes(RES, LOWER, batch=len(seeds))
    first.close()
    gen = cluster.ClusterGenerator(grid.shape, max_batch=MAX_BATCH, cluster_capacity=50000, candidate_capacity=10000)
    gen.set_map(grid)
    gen.build_distance_field()
    field = gen.distance_field()
    gen.polygon_generation(seeds, fetch_clusters=False)
    goals = free[rng.integers(len(free), size=40)].astype(np.int32)
    fan = gen.grid_paths_fan(s[:2], goals, np.arange(40, dtype=np.int32) % 2, path_capacity=512, mem="device")   # the first path call of this handle
    cor = gen.cube_corridors(fan["path_xyz"], fan["path_len"], LOWER, RES, seg_capacity=16)
    kept = {k: v.clone() for k, v in cor.items()}
    fan2 = gen.grid_paths_fan(s[:2], goals, np.arange(40, dtype=np.int32) % 2, 0, pen, path_capacity=512)
    got_hull = gen.hull_planes(RES, LOWER, batch=len(seeds))
    plain, clear = gen.grid_paths(s, g, path_capacity=512), gen.grid_paths_clear(s, g, 0, pen, path_capacity=512)
    torch.cuda.synchronize()
    for k in kept:
        assert torch.equal(kept[k], cor[k]), k
    assert np.array_equal(gen.distance_field(), field) and np.array_equal(gen.get_map(), grid)
    assert (fan["rtn"].cpu().numpy() == fh.OK).sum() >= 20 and (fan2["rtn"] == fh.OK).sum() >= 20 and (want_hull["rtn"] == cluster.HULL_OK).all()
    for k in ("rtn", "n_planes", "n_vertices", "degenerate", "center"):
        assert np.array_equal(want_hull[k], got_hull[k]), k
    for b in range(len(seeds)):
        for k in ("planes", "plane_int", "vertices"):
            assert np.array_equal(want_hull[k][b], got_hull[k][b]), (k, b)
    assert pack(plain, False, cap=512) == pack(want_plain, False, cap=512) and pack(clear, True, cap=512) == pack(want_clear, True, cap=512)
    # a new map: the fan sees it
    before = gen.grid_paths_fan(s[:1], goals[:8], path_capacity=512)
    wall = grid.copy()
    mid = (int(s[0][0]) + 3) % grid.shape[0]
    wall[mid, :, :] = 1
    wall[tuple(s[0])] = 0
    gen.set_map(wall)
    after = gen.grid_paths_fan(s[:1], goals[:8], path_capacity=512)
    pair = gen.grid_paths(np.repeat(s[:1], 4, axis=0), goals[:4], path_capacity=512)
    gen.close()
    assert pack(dict(paths=after["paths"][:4], **{k: after[k][:4] for k in ("rtn", "path_len", "path_cost")}), False, cap=512) == pack(pair, False, cap=512)
    assert pack(before, False, cap=512) != pack(after, False, cap=512)


def test_chain_on_the_device_into_the_optimiser(built):
    """8.  set_map_from_cloud -> grid_paths_fan(mem="device") -> cube_corridors -> direct_ddp_plan_batch (T0 == NULL), 96 goals from one
    source, runs device-resident and gives the bytes of the same arrays routed through host memory.  The plumbing and the layout are
    under test, not the solver: no return code is asked for."""
    import torch
    RES, LOWER = 0.25, np.array([-5.0, -3.0, 0.0])
    dev = "cuda:0"
    N, P, NG = 12, 6, 96
    cloud = (np.argwhere(ch.gap_map() == 1) * RES + 0.5 * RES + LOWER).astype(np.float32)
    gen = cluster.ClusterGenerator(ch.gap_map().shape, max_batch=MAX_BATCH, cluster_capacity=64, candidate_capacity=64)
    gen.set_map_from_cloud(torch.from_numpy(cloud).to(dev), LOWER, RES, cloud_margin=0.0)
    grid = gen.get_map()
    free = np.argwhere(grid == 0)
    rng = np.random.default_rng(6)
    source = np.array([[2, 12, 6]], np.int32)
    goals = free[rng.integers(len(free), size=NG)].astype(np.int32)
    assert grid[2, 12, 6] == 0
    paths = gen.grid_paths_fan(source, goals, path_capacity=64, mem="device")
    host_paths = gen.grid_paths_fan(source, goals, path_capacity=64)
    cor = gen.cube_corridors(paths["path_xyz"], paths["path_len"], LOWER, RES, seg_capacity=N, p_max=P)
    xyz = np.zeros((NG, 64, 3), np.int32)
    for q in range(NG):
        xyz[q, :len(host_paths["paths"][q])] = host_paths["paths"][q]
    host_cor = gen.cube_corridors(xyz, host_paths["path_len"], LOWER, RES, seg_capacity=N, p_max=P)
    gen.close()
    assert paths["path_len"].cpu().numpy().tobytes() == host_paths["path_len"].tobytes()
    for k in abi.CUBE_CORRIDOR_OUTPUTS:
        assert cor[k].cpu().numpy().tobytes() == host_cor[k].tobytes(), k
    ok = (cor["rtn"] == cluster.CUBE_CORRIDOR_OK) & (cor["n_seg"] >= 2)
    pick = torch.nonzero(ok).flatten()
    B = int(pick.numel())
    assert B >= 8, (cor["rtn"].cpu(), cor["n_seg"].cpu(), paths["rtn"].cpu())
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
    print("chain: %d of %d rows, rtn counts %s" % (B, NG, np.unique(r1.rtn, return_counts=True)))
    for dv, hv in ((d0, r0), (d1, r1)):
        for k in ("rtn", "iter_used", "fwd_passes", "cost", "T", "bez", "poly"):
            assert np.asarray(getattr(dv, k)).tobytes() == np.asarray(getattr(hv, k)).tobytes(), k
    assert (h["n_seg"] <= N).all()
