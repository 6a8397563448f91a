"""The corridor kernels (direct_amd/csrc/cluster_corridor.h, cube_corridor.h) where their strided loops take a second trip, on the
device through the C-ABI: polytopes of more than 64 planes in the walk's plane test, paths of more than 64 points, corridors of
more than 64 polytopes, seg_capacity above 64 and above 256, batches of more than 1024 rows through the one-workgroup compaction
of k_corr_unique, and more slots than k_cube_inflate's fixed grid covers.  The inputs are tests/corridor_stride_lib.py's, and
tests/test_corridor_strides_cpp.py asserts on the CPU that each reaches its path.  The references are the g++ harnesses of the
rule headers and oracle.corridor_walk; every comparison is dtype, shape and bytes, and the stats are the harness's."""
import ctypes as C

import numpy as np
import pytest

from direct_amd import abi, cluster
from tests import cluster_corridor_harness as kh
from tests import corridor_lib as lib
from tests import corridor_stride_lib as sl
from tests import cube_corridor_clear_harness as cl
from tests import cube_corridor_harness as ch

pytestmark = pytest.mark.gpu
RES, LOWER = ch.RES, ch.LOWER
KEYS, CUBE_KEYS = kh.KEYS, abi.CUBE_CORRIDOR_OUTPUTS
DEV = "cuda:0"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return sl.build_harness("cluster", tmp_path_factory, "gpu_")


@pytest.fixture(scope="module")
def cube_harness(tmp_path_factory):
    return sl.build_harness("cube", tmp_path_factory, "gpu_")


@pytest.fixture(scope="module")
def clear_harness(tmp_path_factory):
    return sl.build_harness("clear", tmp_path_factory, "gpu_")


def make_gen(grid, max_batch=64):
    g = cluster.ClusterGenerator(ch.DIMS, max_batch=max_batch, cluster_capacity=kh.CAPACITY, candidate_capacity=kh.CAPACITY)
    g.set_map(grid)
    return g


@pytest.fixture(scope="module")
def gen_balls(built):
    g = make_gen(sl.two_ball_map())
    yield g
    g.close()


@pytest.fixture(scope="module")
def gen_crafted(built):
    g = make_gen(ch.crafted_map())
    yield g
    g.close()


@pytest.fixture(scope="module")
def gen_cube(built):
    """the cube corridors' handle: the random map and its uncapped distance field"""
    g = cluster.ClusterGenerator(ch.DIMS, max_batch=64, cluster_capacity=2100, candidate_capacity=64)
    g.set_map(ch.random_map(*sl.CUBE_MAP))
    g.build_distance_field()
    yield g
    g.close()


def on_device(xyz, n):
    import torch
    return torch.from_numpy(xyz).to(DEV), torch.from_numpy(n).to(DEV)


def dirty_call(gen, keys, xyz, n, dtype, pop_back, seg_capacity, p_max=6, itr_cluster_max=None, min_d2=None):
    """the C-ABI call on device memory with every output array PRE-FILLED with 77s: a slot the kernels leave unwritten shows, where
    the wrapper's fresh zeros would pass for the zeros the call owes.  itr_cluster_max: cluster corridors (-> stats as well);
    min_d2: radius-aware cube corridors; neither: cube corridors"""
    import torch
    L = cluster._lib()
    tx, tn = on_device(xyz, n)
    B, cap, S, P = xyz.shape[0], xyz.shape[1], int(seg_capacity), int(p_max)
    real = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    shapes = dict(n_seg=((B,), torch.int32), n_planes=((B, S), torch.int32), planes=((B, S, P, 4), real), seeds=((B, S, 3), real),
                  centers=((B, S, 3), real), cube_idx=((B, S, 6), torch.int32), rtn=((B,), torch.int32))
    out = {k: torch.full(shapes[k][0], 77, dtype=shapes[k][1], device=DEV) for k in keys}
    torch.cuda.synchronize()   # the handle's stream is not torch's
    common = dict(batch=B, path_capacity=cap, mem_in=abi.MEM_DEVICE, itr_inflate_max=1000, path_xyz=tx.data_ptr(), path_len=tn.data_ptr(),
                  pop_back=int(pop_back), seg_capacity=S, p_max=P, plane_dtype=abi.F32 if real == torch.float32 else abi.F64, resolution=RES,
                  map_lower=(C.c_double * 3)(*LOWER))
    ptrs = [out[k].data_ptr() for k in keys]
    stats = np.zeros(4, np.int64)
    if itr_cluster_max is not None:
        par, o = abi.ClusterCorridorIn(itr_cluster_max=int(itr_cluster_max), **common), abi.ClusterCorridorOut(abi.MEM_DEVICE, 0, *ptrs)
        rc = L.direct_cluster_corridor_batch(gen.h, C.addressof(par), C.addressof(o), stats.ctypes.data)
    else:
        par, o = abi.CubeCorridorIn(**common), abi.CubeCorridorOut(abi.MEM_DEVICE, 0, *ptrs)
        if min_d2 is None:
            rc = L.direct_cluster_cube_corridor_batch(gen.h, C.addressof(par), C.addressof(o))
        else:
            rc = L.direct_cluster_cube_corridor_clear_batch(gen.h, C.addressof(par), int(min_d2), C.addressof(o), None)
    assert rc == abi.DIRECT_OK, rc
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if itr_cluster_max is not None:
        res["stats"] = {k: int(v) for k, v in zip(abi.CLUSTER_CORRIDOR_STATS, stats)}
    return res


def cluster_both(gen, harness, xyz, n, table, cases, **kw):
    """the device against the harness for every (dtype, device memory?) of `cases`: bytes and stats.  Host memory goes through the
    wrapper, device memory through dirty_call -> the first case's result"""
    first = None
    for dtype, dev in cases:
        want = kh.corridors(harness, xyz, n, table, dtype=dtype, **kw)
        if dev:
            got = dirty_call(gen, KEYS, xyz, n, dtype, itr_cluster_max=sl.BIG_ITR, **kw)
        else:
            got = gen.cluster_corridors(xyz, n, LOWER, RES, itr_cluster_max=sl.BIG_ITR, dtype=dtype, **kw)
        lib.same(got, want, KEYS)
        assert got["stats"] == want["stats"], (got["stats"], want["stats"])
        first = got if first is None else first
    return first


ALL_CASES = ((np.float64, False), (np.float64, True), (np.float32, False), (np.float32, True))
TWO_CASES = ((np.float64, False), (np.float32, True))   # f64 in host memory, f32 in device memory


# ---- 1. polytopes over 64 planes in the walk ----------------------------------------------------------------------------------

@pytest.mark.parametrize("pop_back", [True, False])
def test_polytopes_over_64_planes_in_the_walk(built, gen_balls, harness, pop_back):
    """polytopes of up to 80 planes on the walk's stack: the device equals the harness and oracle.corridor_walk, both dtypes, host
    and device memory, and a handle with max_batch = 2"""
    rows = sl.wide_rows()
    want, table = kh.oracle_corridors(rows, sl.WIDE_ITR, pop_back, grid=sl.two_ball_map(), tag="two_balls")
    xyz, n = ch.pack_paths(rows, sl.WIDE_CAP)
    kw = dict(pop_back=pop_back, seg_capacity=sl.WIDE_SEG, p_max=sl.WIDE_PMAX)
    got = cluster_both(gen_balls, harness, xyz, n, table, ALL_CASES, **kw)
    ms = gen_balls.last_ms()
    assert (got["rtn"] == kh.OK).all() and got["n_planes"].max() > 64
    kh.assert_rows_equal_oracle(got, want, rows)
    small = make_gen(sl.two_ball_map(), max_batch=2)
    try:
        two = cluster_both(small, harness, xyz, n, table, ((np.float64, False),), **kw)
    finally:
        small.close()
    lib.same(two, got, KEYS)
    print("wide polytopes, %d rows, pop %d: %.3f ms, max planes %d, stats %s" % (len(rows), pop_back, ms, got["n_planes"].max(), got["stats"]))


def test_p_max_64_against_wider_polytopes(gen_balls, harness):
    """p_max = 64: the rows whose corridor has a polytope of more than 64 planes end TOO_MANY_PLANES at the first such, holding the
    head of their full corridor; the others end OK; both occur"""
    rows = sl.wide_rows()
    _, table = kh.oracle_corridors(rows, sl.WIDE_ITR, False, grid=sl.two_ball_map(), tag="two_balls")
    xyz, n = ch.pack_paths(rows, sl.WIDE_CAP)
    full = gen_balls.cluster_corridors(xyz, n, LOWER, RES, itr_cluster_max=sl.WIDE_ITR, pop_back=False, seg_capacity=sl.WIDE_SEG, p_max=sl.WIDE_PMAX)
    assert (full["rtn"] == kh.OK).all()
    few = cluster_both(gen_balls, harness, xyz, n, table, TWO_CASES, pop_back=False, seg_capacity=sl.WIDE_SEG, p_max=64)
    stopped = sl.stopped_at_first_wide(few, full, 64)
    assert 0 < stopped < len(rows)
    print("p_max 64: %d of %d rows stopped, %.3f ms" % (stopped, len(rows), gen_balls.last_ms()))


# ---- 2. paths over 64 points ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pop_back", [True, False])
def test_long_paths_cluster(gen_crafted, harness, pop_back):
    """paths of 64, 65, 128, 129 and 150 points at a path capacity of 150 and seg_capacity 150: harness and oracle; then seg_capacity
    260 on four rows: zeros behind n_seg up to slot 259"""
    rows = sl.long_rows()
    want, table = kh.oracle_corridors(rows, sl.BIG_ITR, pop_back)
    xyz, n = ch.pack_paths(rows, sl.LONG_CAP)
    got = cluster_both(gen_crafted, harness, xyz, n, table, TWO_CASES, pop_back=pop_back, seg_capacity=sl.LONG_CAP, p_max=sl.BIG_PMAX)
    ms = gen_crafted.last_ms()
    assert (got["rtn"] == kh.OK).all()
    kh.assert_rows_equal_oracle(got, want, rows)
    wide = cluster_both(gen_crafted, harness, xyz[:4], n[:4], table, TWO_CASES, pop_back=pop_back, seg_capacity=260, p_max=sl.BIG_PMAX)
    for k in ("n_planes", "planes", "seeds", "centers"):
        assert np.array_equal(wide[k][:, :sl.LONG_CAP], got[k][:4]) and not wide[k][:, sl.LONG_CAP:].any(), k
    print("long paths, cluster, pop %d: %.3f ms, n_seg %s, stats %s" % (pop_back, ms, got["n_seg"].tolist(), got["stats"]))


def test_bad_voxels_behind_point_64_cluster(gen_crafted, harness):
    """the only bad voxel at index 64, 100 or len - 1 = 128, and path_len = capacity + 1: BAD_PATH, n_seg 0 and zeros across the
    seg_capacity of 150; the good rows keep the bytes of the batch without the bad rows"""
    rows = sl.long_rows()
    _, table = kh.oracle_corridors(rows, sl.BIG_ITR, True)
    xyz, n = ch.pack_paths(rows, sl.LONG_CAP)
    kw = dict(pop_back=True, seg_capacity=sl.LONG_CAP, p_max=sl.BIG_PMAX)
    alone = gen_crafted.cluster_corridors(xyz, n, LOWER, RES, itr_cluster_max=sl.BIG_ITR, **kw)
    mx, mn, good_at, bad_at = sl.mix_bad(rows, sl.LONG_CAP)
    got = cluster_both(gen_crafted, harness, mx, mn, table, TWO_CASES, **kw)
    sl.assert_bad_rows_empty(got, bad_at, KEYS)
    assert (got["rtn"][good_at] == kh.OK).all()
    lib.same(lib.pick(got, good_at, KEYS), alone, KEYS)


def cube_both(gen, cube_harness, grid, xyz, n, cases, **kw):
    first = None
    for dtype, dev in cases:
        want = ch.corridors(cube_harness, grid, xyz, n, dtype=dtype, **kw)
        got = dirty_call(gen, CUBE_KEYS, xyz, n, dtype, **kw) if dev else gen.cube_corridors(xyz, n, LOWER, RES, dtype=dtype, **kw)
        lib.same(got, want, CUBE_KEYS)
        first = got if first is None else first
    return first


@pytest.mark.parametrize("pop_back", [True, False])
def test_long_paths_cube(gen_cube, cube_harness, pop_back):
    """cube corridors of up to 87 polytopes at seg_capacity 160; seg_capacity 70, where some rows OVERFLOW with their true n_seg;
    bad voxels behind point 64: BAD_PATH with zeros up to slot 159 beside untouched good rows"""
    grid = ch.random_map(*sl.CUBE_MAP)
    rows = sl.cube_long_rows()
    xyz, n = ch.pack_paths(rows, sl.LONG_CAP)
    got = cube_both(gen_cube, cube_harness, grid, xyz, n, ALL_CASES, pop_back=pop_back, seg_capacity=160)
    ms = gen_cube.last_ms()
    assert (got["rtn"] == ch.OK).all() and got["n_seg"].max() > 64
    cut = cube_both(gen_cube, cube_harness, grid, xyz, n, TWO_CASES, pop_back=pop_back, seg_capacity=70)
    over = got["n_seg"] > 70
    assert cut["rtn"].tolist() == [ch.OVERFLOW if o else ch.OK for o in over] and over.any() and not over.all()
    assert np.array_equal(cut["n_seg"], got["n_seg"])
    mx, mn, good_at, bad_at = sl.mix_bad(rows, sl.LONG_CAP)
    bad = cube_both(gen_cube, cube_harness, grid, mx, mn, TWO_CASES, pop_back=pop_back, seg_capacity=160)
    sl.assert_bad_rows_empty(bad, bad_at, CUBE_KEYS)
    lib.same(lib.pick(bad, good_at, CUBE_KEYS), got, CUBE_KEYS)
    print("long paths, cube, pop %d: %.3f ms, n_seg up to %d" % (pop_back, ms, got["n_seg"].max()))


def test_long_paths_clear(gen_cube, clear_harness):
    """radius-aware cube corridors of the same rows at floor 4, for which the harness still gives corridors of more than 64 (up to
    142) polytopes and every row OK; both walks, f64 in host memory and f32 in device memory"""
    grid = ch.random_map(*sl.CUBE_MAP)
    d2 = cl.brute_d2(grid)
    assert np.array_equal(gen_cube.distance_field(), d2)
    xyz, n = ch.pack_paths(sl.cube_long_rows(), sl.LONG_CAP)
    for pop_back, (dtype, dev) in zip((False, True), TWO_CASES):
        want = cl.corridors(clear_harness, grid, d2, sl.CLEAR_FLOOR, xyz, n, pop_back=pop_back, seg_capacity=160, dtype=dtype)
        if dev:
            got = dirty_call(gen_cube, CUBE_KEYS, xyz, n, dtype, pop_back, 160, min_d2=sl.CLEAR_FLOOR)
        else:
            got = gen_cube.cube_corridors_clear(xyz, n, LOWER, RES, sl.CLEAR_FLOOR, pop_back=pop_back, seg_capacity=160, dtype=dtype)
        lib.same(got, want, CUBE_KEYS)
        assert (got["rtn"] == ch.OK).all() and got["n_seg"].max() > 64
        print("long paths, floor %d, pop %d: %.3f ms, n_seg up to %d" % (sl.CLEAR_FLOOR, pop_back, gen_cube.last_ms(), got["n_seg"].max()))


# ---- 3. batches over 1024 rows -------------------------------------------------------------------------------------------------

BIG_KW = dict(seg_capacity=sl.BIG_SEG, p_max=sl.BIG_PMAX)


@pytest.fixture(scope="module")
def big_tables():
    """the oracle table of the pool, per pop setting: prefixes ask for seeds their rows ask for"""
    return {pop_back: kh.oracle_corridors(sum(sl.big_pool(), []), sl.BIG_ITR, pop_back)[1] for pop_back in (True, False)}


@pytest.mark.parametrize("pop_back", [True, False])
@pytest.mark.parametrize("size", sl.BIG_SIZES)
def test_big_batches(gen_crafted, harness, big_tables, size, pop_back):
    """1025, 2048 and 2500 rows - base rows, prefixes and bad rows, owners on both sides of row 1024: bytes and stats of the harness,
    f64 in host memory and f32 in device memory"""
    xyz, n = ch.pack_paths(sl.big_batch(size), sl.BIG_CAP)
    got = cluster_both(gen_crafted, harness, xyz, n, big_tables[pop_back], TWO_CASES, pop_back=pop_back, **BIG_KW)
    s = got["stats"]
    assert s["unique_seeds"] < s["due_seeds"] and set(got["rtn"].tolist()) == {kh.OK, kh.BAD_PATH}
    print("%d rows, pop %d: %.3f ms, stats %s" % (size, pop_back, gen_crafted.last_ms(), s))


def test_big_batch_shape_independence(built, gen_crafted, harness, big_tables):
    """2500 rows: max_batch = 2 against 64 gives identical bytes; a permutation of the rows gives the permuted bytes; and the call
    again after a call of four rows - the used workspace - gives the first bytes"""
    xyz, n = ch.pack_paths(sl.big_batch(2500), sl.BIG_CAP)
    run = lambda g, a, b: g.cluster_corridors(a, b, LOWER, RES, itr_cluster_max=sl.BIG_ITR, pop_back=True, **BIG_KW)
    one = run(gen_crafted, xyz, n)
    lib.same(one, kh.corridors(harness, xyz, n, big_tables[True], pop_back=True, **BIG_KW), KEYS)
    small = make_gen(ch.crafted_map(), max_batch=2)
    try:
        two = run(small, xyz, n)
        ms = small.last_ms()
    finally:
        small.close()
    lib.same(two, one, KEYS)
    assert two["stats"] == one["stats"]
    perm = np.random.default_rng(1).permutation(len(n))
    assert (perm[:1024] >= 1024).any() and (perm[1024:] < 1024).any()
    p = run(gen_crafted, xyz[perm], n[perm])
    lib.same(p, lib.pick(one, perm, KEYS), KEYS)
    assert {k: v for k, v in p["stats"].items()} == one["stats"]
    four = run(gen_crafted, xyz[:4], n[:4])
    lib.same(four, lib.pick(one, slice(0, 4), KEYS), KEYS)
    again = run(gen_crafted, xyz, n)
    lib.same(again, one, KEYS)
    assert again["stats"] == one["stats"]
    print("2500 rows: %.3f ms at max_batch 64, %.3f ms at max_batch 2, stats %s" % (gen_crafted.last_ms(), ms, one["stats"]))


# ---- 4. cube inflation beyond its fixed grid -----------------------------------------------------------------------------------

def test_inflate_slots_beyond_the_fixed_grid(gen_cube, cube_harness):
    """4100 rows x 128 points = 524800 slots: rows 4096 .. 4099 get their cubes in the strided part of k_cube_inflate and end
    OVERFLOW at seg_capacity 16 with their true n_seg and their first 16 polytopes; every byte equals the harness"""
    xyz, n, bad_at = sl.inflate_batch()
    assert xyz.shape[0] * xyz.shape[1] > sl.INFL_GRID_SLOTS
    got = cube_both(gen_cube, cube_harness, ch.random_map(*sl.CUBE_MAP), xyz, n, ((np.float64, False),), pop_back=True, seg_capacity=sl.INFL_SEG)
    assert (got["rtn"][4096:] == ch.OVERFLOW).all() and (got["n_seg"][4096:] > sl.INFL_SEG).all() and (got["n_planes"][4096:] == 6).all()
    assert (got["rtn"][bad_at] == ch.BAD_PATH).all()
    print("inflate, %d slots: %.3f ms, n_seg of the last rows %s" % (xyz.shape[0] * xyz.shape[1], gen_cube.last_ms(), got["n_seg"][4096:].tolist()))
