"""direct_cluster_cube_corridor_clear_batch (include/direct_cluster.h, "radius-aware cube corridors"; k_floor_fill in
direct_amd/csrc/cube_corridor_clear.h) on the device, through the C-ABI: against the g++ build of the same arithmetic
(tests/cube_corridor_clear_harness.py on the program of tests/cube_corridor_harness.py), against the independent witness - the PLAIN call on a second handle that holds the
thresholded field as its map -, neutral mode, the refusals, the cache of floor tables, launch-shape independence, what the call
leaves alone, the device-resident chain into direct_ddp_plan_batch, and the C++ mirror."""
import functools
import struct

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import corridor_lib as lib
from tests import cube_corridor_clear_harness as cl
from tests import cube_corridor_harness as ch

pytestmark = pytest.mark.gpu
RES, LOWER = ch.RES, ch.LOWER
KEYS = abi.CUBE_CORRIDOR_OUTPUTS
CAP, SEG = 40, 40
BELOW = {4: 1243, 9: 2523, 16: 3669}   # (d2 < floor).sum() on the crafted map
same = functools.partial(lib.same, keys=KEYS)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return cl.build(tmp_path_factory.mktemp("cube_corridor_clear_gpu"))


@pytest.fixture(scope="module")
def gen(built):
    """one handle of ch.DIMS with the crafted map and its uncapped field; every test leaves it that way"""
    g = cluster.ClusterGenerator(ch.DIMS, max_batch=64, cluster_capacity=2100, candidate_capacity=64)
    g.set_map(ch.crafted_map())
    g.build_distance_field()
    yield g
    g.close()


@pytest.fixture(scope="module")
def d2(gen):
    """the reference field, computed once: NumPy brute force, which the device's field equals"""
    want = cl.brute_d2(ch.crafted_map())
    assert np.array_equal(gen.distance_field(), want)
    assert {f: int((want < f).sum()) for f in BELOW} == BELOW
    return want


@pytest.fixture(scope="module")
def rows():
    return lib.rows40()


def test_device_equals_the_clear_harness(gen, harness, rows, d2):
    """1.  every output, bit for bit: host and device memory, both dtypes, both walks, floors 2, 4 and 9, p_max = 7; the three bad
    rows of outside_voxel are BAD_PATH and the rows beside them unaffected"""
    import torch
    grid = ch.crafted_map()
    bad = next(c for c in ch.named_cases() if c["name"] == "outside_voxel")["paths"]
    xyz, n = ch.pack_paths(rows + bad, CAP)
    txyz, tn = torch.from_numpy(xyz).to("cuda:0"), torch.from_numpy(n).to("cuda:0")
    for floor in (2, 4, 9):
        for pop_back, dtype in ((True, np.float64), (False, np.float64), (True, np.float32), (False, np.float32)):
            want = cl.corridors(harness, grid, d2, floor, xyz, n, pop_back=pop_back, seg_capacity=SEG, p_max=7, dtype=dtype)
            host = gen.cube_corridors_clear(xyz, n, LOWER, RES, floor, pop_back=pop_back, seg_capacity=SEG, p_max=7, dtype=dtype)
            same(host, want)
            dev = gen.cube_corridors_clear(txyz, tn, LOWER, RES, floor, pop_back=pop_back, seg_capacity=SEG, p_max=7, dtype=dtype)
            assert all(dev[k].is_cuda for k in KEYS) and isinstance(dev["info"], np.ndarray)
            same(lib.to_host(dev), want)
            assert want["rtn"][:len(rows)].tolist() == [ch.OK] * len(rows) and (want["rtn"][len(rows):] == ch.BAD_PATH).sum() == 3
            assert host["info"][1] == dev["info"][1] == (d2 < floor).sum()
        print("floor %d: %.3f ms, %d polytopes, up to %d per row" % (floor, gen.last_ms(), want["n_seg"].sum(), want["n_seg"].max()))


@pytest.mark.parametrize("floor", [4, 9])
def test_independent_witness_on_the_device(gen, rows, floor):
    """2.  a second handle gets the thresholded field as its map; its PLAIN call gives the first handle's clear call byte for byte"""
    xyz, n = ch.pack_paths(rows, CAP)
    other = cluster.ClusterGenerator(ch.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)
    try:
        other.set_map((gen.distance_field() < floor).astype(np.uint8))
        for pop_back in (True, False):
            same(gen.cube_corridors_clear(xyz, n, LOWER, RES, floor, pop_back=pop_back, seg_capacity=SEG),
                 other.cube_corridors(xyz, n, LOWER, RES, pop_back=pop_back, seg_capacity=SEG))
    finally:
        other.close()


def test_neutral_mode(rows):
    """3.  min_d2 0 and 1 give the plain call's bytes with no field ever built and with a stale one; nothing is built, and the table
    in use counts the occupied voxels"""
    xyz, n = ch.pack_paths(rows, CAP)
    g = cluster.ClusterGenerator(ch.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)
    try:
        g.set_map(ch.crafted_map())
        want = g.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG)
        for stale in (False, True):
            if stale:
                g.build_distance_field()
                assert g.cube_corridors_clear(xyz, n, LOWER, RES, 4, seg_capacity=SEG)["info"].tolist() == [1, BELOW[4]]
                g.set_map(ch.crafted_map())   # the field no longer counts as describing the map
            for floor in (0, 1):
                got = g.cube_corridors_clear(xyz, n, LOWER, RES, floor, seg_capacity=SEG)
                same(got, want)
                assert got["info"].tolist() == [0, 325]
            with pytest.raises(solver.DirectError) as e:
                g.cube_corridors_clear(xyz, n, LOWER, RES, 2, seg_capacity=SEG)
            assert e.value.status == abi.DIRECT_ERR_INVALID and "distance field" in str(e.value)
    finally:
        g.close()


def test_refusals(gen, rows):
    """4.  each DIRECT_ERR_INVALID with nothing written: no field, a stale field, a floor above the cap2 of a capped field (the
    floor AT the cap succeeds and equals the uncapped field's result), a negative floor, and what the plain call refuses"""
    L = cluster._lib()
    xyz, n = ch.pack_paths(rows[:4], CAP)
    info = np.full(2, 77, np.int64)

    def entry(h, par, o, min_d2=4, info=info.ctypes.data):
        return L.direct_cluster_cube_corridor_clear_batch(h, par, min_d2, o, info)

    raw = lib.RawCall(gen, entry, cluster.CubeCorridorIn, cluster.CubeCorridorOut, KEYS, xyz, n, SEG, 6, extras=(info,))
    call, untouched, out = raw.call, raw.untouched, raw.out
    last_error = lambda: L.direct_cluster_last_error().decode()
    for kw in [dict(min_d2=-1), dict(min_d2=-2 ** 31)] + lib.INVALID:
        for floor in ((kw["min_d2"],) if "min_d2" in kw else (0, 4)):   # the plain call's refusals in neutral and in clear mode
            assert call(**dict(kw, min_d2=floor)) == abi.DIRECT_ERR_INVALID, kw
            assert untouched(), kw
    with lib.handle_without_map() as fresh:
        assert call(h=fresh.h) == abi.DIRECT_ERR_INVALID and "no map" in last_error()
        fresh.set_map(ch.crafted_map())
        assert call(h=fresh.h) == abi.DIRECT_ERR_INVALID and "distance field" in last_error()   # no field
        assert untouched()
        fresh.build_distance_field()
        fresh.set_map(ch.crafted_map())
        assert call(h=fresh.h) == abi.DIRECT_ERR_INVALID and "distance field" in last_error()   # a stale one
        assert untouched()
        fresh.build_distance_field(cap_vox=3)
        assert call(h=fresh.h, min_d2=10) == abi.DIRECT_ERR_INVALID and "cap2" in last_error()
        assert untouched()
        assert call(h=fresh.h, min_d2=9) == abi.DIRECT_OK and info.tolist() == [1, BELOW[9]]
        capped = {k: v.copy() for k, v in out.items()}
    assert call(min_d2=9) == abi.DIRECT_OK and (out["rtn"] == cluster.CUBE_CORRIDOR_OK).all()
    same(out, capped)
    # a NULL info and NULL outputs are left alone: only the codes
    status, only = raw.only_codes(info=None)
    assert status == abi.DIRECT_OK and not only.any()


def test_cache_of_floor_tables(rows):
    """5.  by info[0]: the floors 4, 4, 9, 4, 16, 4, 9 build 1, 0, 1, 0, 1, 0, 1; a rebuilt field makes the next call build again
    with unchanged bytes; info[1] is the number of voxels below the floor each time"""
    xyz, n = ch.pack_paths(rows, CAP)
    g = cluster.ClusterGenerator(ch.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)
    try:
        g.set_map(ch.crafted_map())
        g.build_distance_field()
        first = {}
        built = []
        for floor in (4, 4, 9, 4, 16, 4, 9):
            r = g.cube_corridors_clear(xyz, n, LOWER, RES, floor, seg_capacity=SEG)
            built.append(int(r["info"][0]))
            assert r["info"][1] == BELOW[floor]
            same(r, first.setdefault(floor, r))   # a reused table and a rebuilt one give the bytes of the first
        assert built == [1, 0, 1, 0, 1, 0, 1]
        assert first[4]["cube_idx"].tobytes() != first[9]["cube_idx"].tobytes() != first[16]["cube_idx"].tobytes()
        g.build_distance_field()
        for floor, want in ((4, 1), (9, 1), (4, 0), (9, 0)):
            r = g.cube_corridors_clear(xyz, n, LOWER, RES, floor, seg_capacity=SEG)
            assert r["info"].tolist() == [want, BELOW[floor]]
            same(r, first[floor])
    finally:
        g.close()


def test_launch_shape_independence_and_bystanders(gen, rows):
    """6.  one call, two halves and a permuted batch give identical bytes; resident clusters, a grid-path result, the field and the
    PLAIN call's result from before are what they are after"""
    xyz, n = ch.pack_paths(rows, CAP)
    want_plain = gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG)
    by = lib.Bystanders(gen)

    one = gen.cube_corridors_clear(xyz, n, LOWER, RES, 4, seg_capacity=SEG)
    h = len(rows) // 2
    a = gen.cube_corridors_clear(xyz[:h], n[:h], LOWER, RES, 4, seg_capacity=SEG)
    b = gen.cube_corridors_clear(xyz[h:], n[h:], LOWER, RES, 4, seg_capacity=SEG)
    same({k: np.concatenate([a[k], b[k]]) for k in KEYS}, one)
    perm = np.random.default_rng(1).permutation(len(rows))
    same(gen.cube_corridors_clear(xyz[perm], n[perm], LOWER, RES, 4, seg_capacity=SEG), {k: one[k][perm] for k in KEYS})
    gen.cube_corridors_clear(by.dev_path["path_xyz"], by.dev_path["path_len"], LOWER, RES, 9, seg_capacity=SEG)
    same(gen.cube_corridors_clear(xyz, n, LOWER, RES, 4, seg_capacity=SEG), one)

    by.check()
    same(gen.cube_corridors(xyz, n, LOWER, RES, seg_capacity=SEG), want_plain)
    assert one["cube_idx"].tobytes() != want_plain["cube_idx"].tobytes()


def test_chain_on_the_device_into_the_optimiser(built):
    """7.  set_map_from_cloud -> build_distance_field -> grid_paths_fan(min_d2 = 4, device) -> cube_corridors_clear(min_d2 = 4)
    (device in, device out) -> direct_ddp_plan_batch with device inputs and T0 = NULL gives the bytes of the same arrays passed
    through host memory (the plumbing and the layout are under test, not the solver: no return code is asked for); the integer
    guarantee holds on the device's cube_idx, and every path voxel but the start is at or above the floor by path_d2."""
    import torch
    dev = "cuda:0"
    N, P, FLOOR = 12, 6, 4
    occupied = np.argwhere(ch.crafted_map() == 1)
    cloud = (occupied * RES + 0.5 * RES + LOWER).astype(np.float32)
    gen = cluster.ClusterGenerator(ch.DIMS, max_batch=16, cluster_capacity=64, candidate_capacity=64)
    gen.set_map_from_cloud(torch.from_numpy(cloud).to(dev), LOWER, RES, cloud_margin=0.0)
    gen.build_distance_field()
    d2 = gen.distance_field()   # of the map the cloud gave (float32 points: not voxel for voxel the crafted map)
    assert np.array_equal(d2 == 0, gen.get_map() == 1)
    open_ = np.argwhere(d2 >= FLOOR)
    rng = np.random.default_rng(6)
    sources = open_[rng.integers(len(open_), size=2)].astype(np.int32)
    goals = open_[rng.integers(len(open_), size=16)].astype(np.int32)
    goal_src = (np.arange(16) % 2).astype(np.int32)
    paths = gen.grid_paths_fan(sources, goals, goal_src, min_d2=FLOOR, path_capacity=64, mem="device")
    cor = gen.cube_corridors_clear(paths["path_xyz"], paths["path_len"], LOWER, RES, FLOOR, seg_capacity=N, p_max=P)
    gen.close()
    assert cor["info"].tolist() == [1, int((d2 < FLOOR).sum())]
    ok = (cor["rtn"] == cluster.CUBE_CORRIDOR_OK) & (cor["n_seg"] >= 2)
    pick = torch.nonzero(ok).flatten()[:6]
    B = int(pick.numel())
    assert B >= 2, (cor["rtn"].cpu(), cor["n_seg"].cpu(), paths["rtn"].cpu())
    # the guarantee, on what the device wrote
    hc = lib.to_host({k: cor[k] for k in KEYS})
    plen, pd2 = paths["path_len"].cpu().numpy(), paths["path_d2"].cpu().numpy()
    good = np.flatnonzero(hc["rtn"] == cluster.CUBE_CORRIDOR_OK)
    checked, large = cl.guarantee(hc["cube_idx"][good], hc["n_seg"][good], np.rint((hc["seeds"][good] - LOWER) / RES - 0.5).astype(int), d2, FLOOR)
    assert checked >= 2 * B and large >= 1
    for b in np.flatnonzero(paths["rtn"].cpu().numpy() == cluster.GRID_PATH_OK):
        assert (pd2[b, 1:plen[b]] >= FLOOR).all(), b
    x0, xd = lib.chain_ends(paths, pick)
    h, (_, r1), _ = lib.plan_chain({k: cor[k][pick] for k in ("n_seg", "n_planes", "planes", "seeds")}, x0, xd, N, P)
    print("chain: %d rows, n_seg %s, rtn %s" % (B, h["n_seg"].tolist(), r1.rtn.tolist()))
    assert (h["n_seg"] <= N).all()


def test_cpp_mirror_against_the_python_call(gen, rows, tmp_path):
    """8.  polyhedronGenerator::cubeCorridorClearBatch (direct_amd/host/poly_utils.hpp) fills its corridors with the planes, centres
    and seeds of cube_corridors_clear, bit for bit, for both walks (tests/cpp/test_cube_corridor_clear_gen.cpp)"""
    FLOOR = 4
    xyz, n = ch.pack_paths(rows, CAP)
    tail = struct.pack("<2i", FLOOR, CAP)
    for pop_back in (True, False):
        r = gen.cube_corridors_clear(xyz, n, LOWER, RES, FLOOR, pop_back=pop_back, seg_capacity=CAP)
        assert (r["rtn"] == cluster.CUBE_CORRIDOR_OK).all()
        tail += b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("n_seg", "planes", "centers", "seeds"))
    lib.run_cpp_mirror(tmp_path, "test_cube_corridor_clear_gen.cpp", rows, tail)
