"""direct_cluster_free_components / direct_cluster_get_free_components / direct_cluster_reachable_batch (include/direct_cluster.h,
"free-space components"; kernels in direct_amd/csrc/free_comp.h) on the device, through the C-ABI: against the g++ build of the
same rules (tests/free_comp_harness.py), against the path calls as an independent witness, launch-shape and history independence,
staleness, what a build leaves alone, and the C++ mirror."""
import os
import struct
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import dist_field_harness as dh
from tests import free_comp_harness as fh

pytestmark = pytest.mark.gpu
ROOT = fh.ROOT
OK, NO_PATH, BAD, OVERFLOW, ROUND_LIMIT = (cluster.GRID_PATH_OK, cluster.GRID_PATH_NO_PATH, cluster.GRID_PATH_BAD_ENDPOINT,
                                           cluster.GRID_PATH_OVERFLOW, cluster.GRID_PATH_ROUND_LIMIT)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return fh.build(tmp_path_factory.mktemp("free_comp_gpu"))


def handle(grid, field=False, cap_vox=0, max_batch=4):
    gen = cluster.ClusterGenerator(grid.shape, max_batch=max_batch, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
    if field:
        gen.build_distance_field(cap_vox)
    return gen


def stats_list(s):
    return [s["enterable"], s["components"], s["largest"], s["largest_label"]]


def check_device(gen, want, min_d2, what):
    """a build on the device against the g++ result `want`: stats, and labels and sizes through both memory kinds of the fetch"""
    stats = gen.build_free_components(min_d2)
    assert stats_list(stats) == want["stats"].tolist(), (what, stats, want["stats"])
    label, size = gen.free_components()
    assert label.dtype == np.int32 and label.tobytes() == want["label"].tobytes(), what
    assert size.tobytes() == want["size"].tobytes(), what
    dl, ds = gen.free_components(mem="device")
    assert dl.is_cuda and dl.cpu().numpy().tobytes() == want["label"].tobytes() and ds.cpu().numpy().tobytes() == want["size"].tobytes(), what
    assert gen.free_components_floor() == (0 if min_d2 <= 1 else min_d2)


def refused(call, word):
    with pytest.raises(solver.DirectError) as e:
        call()
    return e.value.status == abi.DIRECT_ERR_INVALID and word in str(e.value)


def test_device_equals_the_header_on_every_map(built, exe):
    """1.  labels, sizes and stats of the named, degenerate and random maps equal the g++ build byte for byte, in both memory kinds"""
    for name, grid in fh.named_maps() + fh.degenerate_maps() + fh.random_maps():
        gen = handle(grid)
        try:
            check_device(gen, fh.run(exe, grid), 0, name)
            print("%s: %.3f ms" % (name, gen.last_ms()))
        finally:
            gen.close()


@pytest.mark.parametrize("width", [1, 3, 5])
def test_device_equals_the_header_under_a_floor(built, exe, width):
    """1.  the door maps at the floor that separates the rooms and the one below, on the uncapped and on a capped field; min_d2 = 1 is
    the plain graph; a floor above cap2, a missing and a stale field are refused with the clear path call's words"""
    grid = fh.door_map(width)
    d2 = dh.brute_d2(grid)
    floor = fh.separating_floor(grid, d2)
    gen = handle(grid)
    try:
        assert refused(lambda: gen.build_free_components(floor), "distance field")   # no field ever built
        gen.build_distance_field()
        assert np.array_equal(gen.distance_field(), d2)
        rooms = []
        for f in (floor - 1, floor):
            want = fh.run(exe, grid, d2, f)
            check_device(gen, want, f, ("door", width, f))
            rooms.append(int(want["stats"][1]))
        assert rooms[0] != rooms[1]
        check_device(gen, fh.run(exe, grid), 1, "min_d2 = 1")
        gen.build_distance_field(4)
        for f in (floor - 1, floor):
            check_device(gen, fh.run(exe, grid, d2, f), f, ("capped", width, f))
        assert refused(lambda: gen.build_free_components(17), "cap2")
        gen.set_map(grid)
        assert refused(lambda: gen.build_free_components(floor), "distance field")   # stale
        assert gen.build_free_components(0)["components"] == 1
    finally:
        gen.close()


def test_reachable_equals_the_pair_rule(built, exe):
    """2.  the pairs of the CPU test - occupied starts, s == g on an occupied voxel, a goal beside an occupied start, endpoints
    outside on each side - with host and device inputs and outputs, against the g++ pair rule"""
    import torch
    grid = fh.random_map(fh.DIMS, 1)
    starts, goals = fh.rule_pairs(grid)
    want = fh.run(exe, grid, starts=starts, goals=goals)
    assert {OK, NO_PATH, BAD} == set(want["rtn"].tolist())
    gen = handle(grid)
    try:
        gen.build_free_components()
        host = gen.reachable(starts, goals)
        dev = gen.reachable(torch.from_numpy(starts).to("cuda:0"), torch.from_numpy(goals).to("cuda:0"), mem="device")
        mixed = gen.reachable(torch.from_numpy(starts).to("cuda:0"), torch.from_numpy(goals).to("cuda:0"), mem="host")
        for k, name in enumerate(("rtn", "goal_label", "goal_size")):
            assert host[k].tobytes() == want[name].tobytes(), name
            assert dev[k].is_cuda and dev[k].cpu().numpy().tobytes() == want[name].tobytes(), name
            assert mixed[k].tobytes() == want[name].tobytes(), name
        assert refused(lambda: gen.reachable(starts, goals, min_d2=2), "differs from the floor")
        assert gen.reachable(starts, goals, min_d2=1)[0].tobytes() == want["rtn"].tobytes()   # one normal form
    finally:
        gen.close()


def agree(reach, rtn_p):
    """reachable says OK exactly where the path call says OK or OVERFLOW, and NO_PATH and BAD_ENDPOINT exactly where it does"""
    rtn_p = np.asarray(rtn_p)
    assert (rtn_p != ROUND_LIMIT).all()
    assert np.array_equal(reach == OK, (rtn_p == OK) | (rtn_p == OVERFLOW))
    assert np.array_equal(reach == NO_PATH, rtn_p == NO_PATH) and np.array_equal(reach == BAD, rtn_p == BAD)


def test_path_calls_as_independent_witness(built):
    """3.  grid_paths on 64 pairs of the seed-1 map (a capacity of 6 voxels makes long paths OVERFLOW), grid_paths_clear on a door map
    at the two floors around the separation, and grid_paths_fan with one source and 500 goals in both modes: reachable foretells
    their codes"""
    grid = fh.random_map(fh.DIMS, 1)
    starts, goals = fh.rule_pairs(grid)
    gen = handle(grid, max_batch=64)
    try:
        largest = gen.build_free_components()["largest_label"]
        rtn_p = gen.grid_paths(starts, goals, path_capacity=6)["rtn"]
        assert {OK, NO_PATH, BAD, OVERFLOW} <= set(rtn_p.tolist())
        agree(gen.reachable(starts, goals)[0], rtn_p)
        rng = np.random.default_rng(3)
        many = rng.integers(-1, np.array(fh.DIMS) + 1, (500, 3)).astype(np.int32)   # occupied and outside goals among them
        inside = np.array(np.unravel_index(largest, fh.DIMS), np.int32)   # a source in the largest component, and an occupied one
        for source in (inside, np.argwhere(grid == 1)[7].astype(np.int32)):
            src = np.repeat(source[None], 500, 0)
            fan = gen.grid_paths_fan(source[None], many, path_capacity=64)["rtn"]
            agree(gen.reachable(src, many)[0], fan)
            if source is inside:
                assert (fan == OK).sum() >= 5 and (fan == NO_PATH).sum() >= 5
    finally:
        gen.close()
    door = fh.door_map(3)
    d2 = dh.brute_d2(door)
    floor = fh.separating_floor(door, d2)
    s2, g2 = fh.free_pairs(door, 64, 3)
    s2[:12] = np.argwhere((door == 0) & (d2 < floor))[:12]   # starts below the floor leave through a neighbour
    gen = handle(door, field=True, max_batch=64)
    try:
        seen = set()
        for f in (floor - 1, floor):
            gen.build_free_components(f)
            rtn_p = gen.grid_paths_clear(s2, g2, min_d2=f)["rtn"]
            agree(gen.reachable(s2, g2, min_d2=f)[0], rtn_p)
            seen |= set(rtn_p.tolist())
            many = np.random.default_rng(4).integers(0, np.array(fh.DIMS), (500, 3)).astype(np.int32)
            fan = gen.grid_paths_fan(s2[20:21], many, min_d2=f)["rtn"]
            agree(gen.reachable(np.repeat(s2[20:21], 500, 0), many, min_d2=f)[0], fan)
        assert {OK, NO_PATH} <= seen
        assert (fan == NO_PATH).sum() >= 100 and (fan == OK).sum() >= 100   # at the separating floor: the other room
    finally:
        gen.close()


def test_launch_shape_and_history_independence(built):
    """4.  build, build for another floor, build the first again: identical bytes; n pairs in one call, in two halves and permuted:
    identical per-pair bytes"""
    grid = fh.door_map(3)
    gen = handle(grid, field=True)
    try:
        gen.build_free_components(5)
        first = [a.tobytes() for a in gen.free_components()]
        starts, goals = fh.free_pairs(grid, 300, 9)
        starts[:40] = np.argwhere(grid == 1)[:40]
        one = gen.reachable(starts, goals, min_d2=5)
        gen.build_free_components(0)
        assert [a.tobytes() for a in gen.free_components()] != first
        gen.build_free_components(5)
        assert [a.tobytes() for a in gen.free_components()] == first
        halves = [gen.reachable(starts[a:b], goals[a:b], min_d2=5) for a, b in ((0, 131), (131, 300))]
        perm = np.random.default_rng(1).permutation(300)
        shuffled = gen.reachable(starts[perm], goals[perm], min_d2=5)
        for k in range(3):
            assert np.concatenate([h[k] for h in halves]).tobytes() == one[k].tobytes()
            assert shuffled[k].tobytes() == one[k][perm].tobytes()
    finally:
        gen.close()


def test_staleness(built, exe):
    """5.  set_map, set_map_from_cloud - a failing one included - and, for labels built with a floor, build_distance_field make the
    labels stale: the fetch and reachable refuse; a rebuild serves again and follows the new map"""
    grid, other = fh.door_map(3), fh.random_map(fh.DIMS, 2)
    s, g = fh.free_pairs(other, 8, 2)
    gen = handle(grid, field=True)
    stale = lambda: refused(gen.free_components, "no valid free components") and refused(lambda: gen.reachable(s, g), "no valid free components")
    try:
        assert refused(gen.free_components, "no valid free components")   # never built
        gen.build_free_components()
        gen.build_distance_field()          # labels built without a floor never looked at the field
        gen.free_components()
        gen.set_map(other)
        assert stale()
        check_device(gen, fh.run(exe, other), 0, "after set_map")
        with pytest.raises(solver.DirectError):
            gen.set_map_from_cloud(np.zeros((4, 3), np.float32), (0, 0, 0), -1.0)   # refused: the map is untouched, the labels still go
        assert stale()
        gen.build_free_components()
        gen.set_map_from_cloud(np.zeros((0, 3), np.float32), (0, 0, 0), 0.1)         # an empty cloud: the empty map
        assert stale()
        assert stats_list(gen.build_free_components()) == [5760, 1, 5760, 0]
        gen.set_map(grid)
        gen.build_distance_field()
        gen.build_free_components(5)
        gen.reachable(s, g, min_d2=5)
        gen.build_distance_field()
        assert refused(lambda: gen.reachable(s, g, min_d2=5), "no valid free components") and refused(gen.free_components, "no valid")
        assert gen.build_free_components(5)["components"] == 2
    finally:
        gen.close()


def test_neighbours_untouched(built):
    """6.  resident clusters, a grid-path result, the distance field and a floor table are byte-identical before and after a build"""
    grid = fh.door_map(5)
    gen = cluster.ClusterGenerator(grid.shape, max_batch=4, cluster_capacity=4096, candidate_capacity=1024)
    try:
        gen.set_map(grid)
        gen.build_distance_field()
        s, g = fh.free_pairs(grid, 4, 6)
        xyz, n = np.zeros((4, 8, 3), np.int32), np.full(4, 1, np.int32)
        xyz[:, 0] = s
        pack = lambda r: [np.asarray(v).tobytes() for v in r.values() if v is not None and not isinstance(v, list)]
        table = gen.cube_corridors_clear(xyz, n, (0, 0, 0), 0.1, 4)
        assert table["info"][0] == 1
        paths = gen.grid_paths(s, g)
        field = gen.distance_field().tobytes()
        gen.polygon_generation(s, fetch_clusters=False)
        hull = gen.hull_planes(0.1, (0, 0, 0), batch=4)
        for floor in (0, 4):
            gen.build_free_components(floor)
        assert gen.distance_field().tobytes() == field
        again = gen.hull_planes(0.1, (0, 0, 0), batch=4)                 # the clusters are still resident
        for k in ("n_planes", "rtn", "center"):
            assert again[k].tobytes() == hull[k].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again["planes"], hull["planes"]))
        reused = gen.cube_corridors_clear(xyz, n, (0, 0, 0), 0.1, 4)
        assert reused["info"][0] == 0 and pack(reused)[:-1] == pack(table)[:-1]   # the floor table served again, unrebuilt
        after = gen.grid_paths(s, g)   # stats, and dist beyond the goal's value, are not deterministic: the contract's outputs
        for k in ("path_len", "path_cost", "rtn"):
            assert after[k].tobytes() == paths[k].tobytes(), k
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after["paths"], paths["paths"]))
    finally:
        gen.close()


def test_cpp_mirror_against_the_python_call(built, tmp_path):
    """7.  polyhedronGenerator::buildFreeComponents / reachable (direct_amd/host/poly_utils.hpp) give the binding's stats, codes and
    sizes, and throw without labels and with stale ones (tests/cpp/test_free_comp_gen.cpp)"""
    RES, LOWER = 0.25, (-3.0, -2.5, 0.0)
    grid = fh.door_map(3)
    fin, exe = str(tmp_path / "in.bin"), str(tmp_path / "gen")
    rng = np.random.default_rng(8)
    vs, vg = rng.integers(0, np.array(fh.DIMS), (2, 200, 3))
    coord = lambda v: (v + rng.random(v.shape) * 0.9 + 0.05) * RES + np.array(LOWER)
    cs, cg = coord(vs), coord(vg)
    gen = handle(grid, field=True)
    try:
        with open(fin, "wb") as f:
            f.write(struct.pack("<3id3d", *fh.DIMS, RES, *LOWER))
            f.write(grid.tobytes())
            f.write(struct.pack("<i", 2))
            for floor in (0, 5):
                stats = gen.build_free_components(floor)
                rtn, _, size = gen.reachable(vs.astype(np.int32), vg.astype(np.int32), min_d2=floor)
                assert {OK, NO_PATH} <= set(rtn.tolist())
                f.write(struct.pack("<i4qi", floor, *stats_list(stats), 200))
                f.write(np.ascontiguousarray(cs, np.float64).tobytes() + np.ascontiguousarray(cg, np.float64).tobytes())
                f.write(rtn.tobytes() + size.tobytes())
    finally:
        gen.close()
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests/cpp/test_free_comp_gen.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "direct_amd/lib"), "-ldirect_ddp",
                           "-Wl,-rpath," + os.path.join(ROOT, "direct_amd/lib") + ":/opt/rocm/lib"])
    out = subprocess.run([exe, fin], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
