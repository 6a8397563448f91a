"""Known space and frontier goals on the device (include/direct_cluster.h, "known space and frontier goals"; kernels in
direct_amd/csrc/map_scan.h and direct_amd/csrc/frontier.h) against the NumPy restatement of tests/frontier_harness.py, which
tests/test_frontier_restatement.py holds equal to the g++ build of the same headers.  Grids are bytes, labels are indices and stats
are counts: everything is compared for equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import dist_field_harness as dh
from tests import free_comp_harness as fh
from tests import frontier_harness as fr
from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh

pytestmark = pytest.mark.gpu
ROOT = sh.ROOT
SMALL = dict(max_batch=4, cluster_capacity=64, candidate_capacity=64)
ORIGIN_VOXEL = (22, 16, 6)


def scan(g, pts, max_range, mode="continue", track=True, inflate=(0, 0, 0)):
    return g.integrate_scan(pts, sh.ORIGIN, sh.LOWER, sh.RES, max_range, inflate=inflate, mode=mode, map_upper=sh.UPPER, track_known=track)


def stats_of(d):
    return [d[k] for k in sh.STATS]


def refused(word, call):
    with pytest.raises(solver.DirectError) as e:
        call()
    assert e.value.status == abi.DIRECT_ERR_INVALID and word in str(e.value), str(e.value)


# ---- tracked scans ------------------------------------------------------------------------------------------------------------
def test_tracked_scans_equal_the_restatement_and_the_untracked_scan(built):
    """n below, at and above one wave and several workgroups, and the lattice cloud, at 1.5 m and 10 m: the known grid, the scan
    grid, the map and the eight stats against the restatement, and the last three against the same scan untracked on a second handle"""
    rnd = mh.cloud_random(1000)
    clouds = {"random_%d" % n: rnd[:n] for n in (0, 1, 63, 64, 65, 1000)}
    clouds["lattice"] = sh.cloud_lattice()
    a, b = cluster.ClusterGenerator(sh.DIMS, **SMALL), cluster.ClusterGenerator(sh.DIMS, **SMALL)
    for g in (a, b):
        g.set_map(np.ones(sh.DIMS, np.uint8))
    for name, pts in clouds.items():
        for r in (1.5, 10.0):
            before = a.get_map()
            raw, new, wstats = sh.restate(pts, sh.ORIGIN, r, (1, 0, 1), before=before)
            sa, sb = scan(a, pts, r, "reset", True, (1, 0, 1)), scan(b, pts, r, "reset", False, (1, 0, 1))
            assert np.array_equal(a.known_grid(), fr.known_restate(pts, sh.ORIGIN, r)), (name, r)
            for g, st in ((a, sa), (b, sb)):
                assert np.array_equal(g.scan_grid(), raw) and np.array_equal(g.get_map(), new) and stats_of(st) == wstats.tolist(), (name, r)
            refused("no known grid", b.known_grid)
    assert a.last_ms() > 0.0
    a.close()
    b.close()


def test_the_three_modes_and_what_drops_the_grid(built):
    pts = mh.cloud_random(900)
    a, b, c = pts[:300], pts[300:600], pts[600:]
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    refused("no known grid", g.known_grid)
    ka = fr.known_restate(a, sh.ORIGIN, 1.5)
    scan(g, a, 1.5)                                                       # CONTINUE on a handle without a known grid starts empty
    assert np.array_equal(g.known_grid(), ka)
    kab = fr.known_restate(b, sh.ORIGIN, 10.0, known=ka)
    scan(g, b, 10.0)                                                      # CONTINUE: the union
    assert np.array_equal(g.known_grid(), kab) and kab.sum() > ka.sum()
    g.set_map(np.ones(sh.DIMS, np.uint8))                                 # set_map leaves it alone
    assert np.array_equal(g.known_grid(), kab)
    g.set_map_from_cloud(c, sh.LOWER, sh.RES, 0.0, map_upper=sh.UPPER)    # ... and so does map_from_cloud
    assert np.array_equal(g.known_grid(), kab)
    adopted = g.get_map()
    st = scan(g, c, 1.5, "adopt")                                         # ADOPT keeps it, and says nothing about what was seen
    assert np.array_equal(g.known_grid(), fr.known_restate(c, sh.ORIGIN, 1.5, known=kab))
    want = sh.restate(c, sh.ORIGIN, 1.5, raw=adopted, before=adopted)
    assert np.array_equal(g.scan_grid(), want[0]) and stats_of(st) == want[2].tolist()
    scan(g, a, 1.5, "reset")                                              # RESET empties it
    assert np.array_equal(g.known_grid(), ka)
    scan(g, b, 10.0, track=False)                                         # an untracked scan drops it
    refused("no known grid", g.known_grid)
    refused("no known grid", g.frontiers)
    scan(g, a, 1.5)                                                       # ... and the next tracked one starts empty
    assert np.array_equal(g.known_grid(), ka)
    with pytest.raises(solver.DirectError):                               # a refused scan leaves it
        scan(g, a, -1.0, track=False)
    assert np.array_equal(g.known_grid(), ka)
    g.close()


def test_set_known_and_get_known(built):
    import torch
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    src = (np.random.default_rng(2).integers(0, 4, sh.DIMS) * (np.random.default_rng(3).random(sh.DIMS) < 0.5)).astype(np.uint8)
    want = (src != 0).astype(np.uint8)
    assert want.any() and (src > 1).any()
    g.set_known(src)
    assert np.array_equal(g.known_grid(), want)
    g.set_known(None)
    assert not g.known_grid().any()
    g.set_known(torch.from_numpy(src).to("cuda:0"))
    out = torch.full(sh.DIMS, 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert cluster._lib().direct_cluster_get_known(g.h, abi.MEM_DEVICE, out.data_ptr()) == abi.DIRECT_OK
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(g.known_grid(), want)
    g.close()


CHILD = """
import sys
import numpy as np
from direct_amd import cluster
from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh
g = cluster.ClusterGenerator(sh.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)
g.set_map(np.ones(sh.DIMS, np.uint8))
st = g.integrate_scan(mh.cloud_random(1000), sh.ORIGIN, sh.LOWER, sh.RES, 1.5, mode="adopt", map_upper=sh.UPPER, track_known=True)
np.savez(sys.argv[1], known=g.known_grid(), raw=g.scan_grid(), stats=np.array([st[k] for k in sh.STATS], np.int64))
g.close()
"""


def test_the_plain_store_leaves_the_same_grids(built, tmp_path):
    """DIRECT_CLUSTER_SCAN_STORE=plain is read at create time from the environment: a fresh child process"""
    out = str(tmp_path / "plain.npz")
    env = dict(os.environ, DIRECT_CLUSTER_SCAN_STORE="plain", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(out)
    pts, full = mh.cloud_random(1000), np.ones(sh.DIMS, np.uint8)
    raw, _, wstats = sh.restate(pts, sh.ORIGIN, 1.5, raw=full, before=full)
    assert np.array_equal(got["known"], fr.known_restate(pts, sh.ORIGIN, 1.5))
    assert np.array_equal(got["raw"], raw) and got["stats"].tolist() == wstats.tolist()


# ---- frontiers ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen(built):
    g = cluster.ClusterGenerator(fh.DIMS, **SMALL)
    yield g
    g.close()


@pytest.mark.parametrize("name", [n for n, _, _ in fr.scenes()])
def test_frontiers_equal_the_restatement(gen, name):
    grid, known = {n: (g, k) for n, g, k in fr.scenes()}[name]
    comp = fr.components(grid, known)
    kept = len(comp["roots"])
    gen.set_map(grid)
    gen.set_known(known)
    for min_size in (1, 5):
        for mem in ("host", "device"):
            got = gen.frontiers(min_size=min_size, mem=mem, voxel_labels=True)
            fr.assert_same(got, fr.select(comp, min_size, 1024), (name, min_size, mem))
    for cap in sorted({0, max(kept - 1, 0), kept + 3}):
        for mem in ("host", "device"):
            fr.assert_same(gen.frontiers(capacity=cap, mem=mem), fr.select(comp, 1, cap), (name, cap, mem))
    assert gen.last_ms() > 0.0


def test_frontiers_with_a_floor(gen):
    grid, known = fr.door_scene(3)
    d2 = dh.brute_d2(grid)
    floor = fh.separating_floor(grid, d2)
    gen.set_map(grid)
    gen.set_known(known)
    gen.build_distance_field()
    for min_d2 in (2, floor):
        comp = fr.components(grid, known, d2, min_d2)
        for min_size, cap in ((1, 1024), (5, 1024), (1, 1)):
            fr.assert_same(gen.frontiers(min_size=min_size, min_d2=min_d2, capacity=cap, voxel_labels=True), fr.select(comp, min_size, cap),
                           (min_d2, min_size, cap))
    assert len(fr.components(grid, known, d2, floor)["roots"]) == 2


def test_the_scan_of_the_workgroup_counts_crosses_a_lane_s_run(built):
    """40 x 36 x 20 voxels are 113 workgroup counts, two words per lane of k_front_scan; hundreds of kept roots spread over them"""
    grid = (np.random.default_rng(5).random(fh.DIMS_BIG) < 0.2).astype(np.uint8)
    known = (np.random.default_rng(6).random(fh.DIMS_BIG) < 0.05).astype(np.uint8)
    comp = fr.components(grid, known)
    assert len(comp["roots"]) > 113
    g = cluster.ClusterGenerator(fh.DIMS_BIG, **SMALL)
    g.set_map(grid)
    g.set_known(known)
    for min_size, cap, mem in ((1, 4096, "host"), (3, 4096, "device"), (1, 200, "host")):
        fr.assert_same(g.frontiers(min_size=min_size, capacity=cap, mem=mem, voxel_labels=True), fr.select(comp, min_size, cap), (min_size, cap))
    g.close()


def test_two_calls_in_a_row_and_the_free_components_around_them(gen):
    """counters and scratch are cleared per call; the labelling uses buffers of its own, so the free-space labels still serve"""
    _, grid, known = fr.scenes()[-2]
    gen.set_map(grid)
    gen.set_known(known)
    gen.build_free_components()
    label, size = (a.tobytes() for a in gen.free_components())
    free = np.argwhere(grid == 0).astype(np.int32)
    ends = free[np.random.default_rng(4).choice(len(free), 16, replace=False)]
    reach = [np.asarray(v).tobytes() for v in gen.reachable(ends[:8], ends[8:])]
    first = gen.frontiers(min_size=2, capacity=40, voxel_labels=True)
    gen.frontiers(min_size=1, capacity=3)                                  # other sizes in between
    second = gen.frontiers(min_size=2, capacity=40, voxel_labels=True)
    assert first["stats"] == second["stats"] and first["stats"]["kept"] > 40
    for k in ("label", "size", "centroid", "rep", "voxel_label"):
        assert first[k].tobytes() == second[k].tobytes(), k
    assert [a.tobytes() for a in gen.free_components()] == [label, size]
    assert [np.asarray(v).tobytes() for v in gen.reachable(ends[:8], ends[8:])] == reach
    assert np.array_equal(gen.known_grid(), (known != 0).astype(np.uint8)) and np.array_equal(gen.get_map(), grid)


# ---- the chain, once ----------------------------------------------------------------------------------------------------------
def test_scan_frontiers_reachable_fan(built):
    wpts, room, _ = sh.wall_and_room()
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    scan(g, wpts, 10.0)
    st = scan(g, room, 10.0)
    assert st["set"] + st["cleared"] > 0
    f = g.frontiers(min_size=3)
    rep = f["rep"]
    assert len(rep) > 0 and f["stats"]["written"] == f["stats"]["kept"] == len(rep)
    known, grid = g.known_grid(), g.get_map()
    assert all(known[tuple(v)] == 1 and grid[tuple(v)] == 0 for v in rep)
    g.build_free_components()
    src = np.tile(np.array(ORIGIN_VOXEL, np.int32), (len(rep), 1))
    rtn, _, _ = g.reachable(src, rep)
    ok = rtn == cluster.GRID_PATH_OK
    assert ok.any()
    out = g.grid_paths_fan(np.array([ORIGIN_VOXEL], np.int32), rep[ok])
    assert (out["rtn"] == cluster.GRID_PATH_OK).all()
    for path, goal in zip(out["paths"], rep[ok]):
        assert np.array_equal(path[0], ORIGIN_VOXEL) and np.array_equal(path[-1], goal)
    g.close()


def test_cpp_mirror_against_the_python_call(built, tmp_path):
    """polyhedronGenerator::integrateScan(track_known) / getKnown / setKnown / frontiers (direct_amd/host/poly_utils.hpp) give the
    binding's known grid, stats and arrays (tests/cpp/test_frontier_gen.cpp)"""
    import struct
    pts = mh.cloud_random(900)
    fin, exe = str(tmp_path / "in.bin"), str(tmp_path / "gen")
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    scan(g, pts, 1.5, "reset")
    calls = ((1, 0, 1024), (3, 0, 1024), (1, 0, 2), (1, 0, 0))
    with open(fin, "wb") as f:
        f.write(struct.pack("<3id3d3ddi", *sh.DIMS, sh.RES, *sh.LOWER, *sh.ORIGIN, 1.5, len(pts)))
        f.write(np.ascontiguousarray(pts, np.float32).tobytes() + g.known_grid().tobytes())
        f.write(struct.pack("<i", len(calls)))
        for min_size, min_d2, cap in calls:
            r = g.frontiers(min_size=min_size, min_d2=min_d2, capacity=cap)
            f.write(struct.pack("<3i", min_size, min_d2, cap) + np.array([r["stats"][k] for k in fr.STATS], np.int64).tobytes())
            f.write(b"".join(np.ascontiguousarray(r[k], np.int32).tobytes() for k in ("label", "size", "centroid", "rep")))
    assert r["stats"]["kept"] >= 1 and r["stats"]["written"] == 0
    g.close()
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests/cpp/test_frontier_gen.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "direct_amd/lib"), "-ldirect_ddp",
                           "-Wl,-rpath," + os.path.join(ROOT, "direct_amd/lib") + ":/opt/rocm/lib"])
    out = subprocess.run([exe, fin], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- refusals on a live handle --------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle(built):
    grid, known = fr.door_scene(3)
    g = cluster.ClusterGenerator(fh.DIMS, **SMALL)
    refused("no map", g.frontiers)
    g.set_map(grid)
    refused("no known grid", g.frontiers)
    g.set_known(known)
    refused("no valid distance field", lambda: g.frontiers(min_d2=4))
    assert g.frontiers(min_d2=1)["stats"]["frontier"] > 0                   # no floor: no field needed
    g.build_distance_field()
    assert g.frontiers(min_d2=4)["stats"]["frontier"] > 0
    g.set_map(grid)                                                        # the field is stale
    for call in (lambda: g.frontiers(min_d2=4), lambda: g.frontiers(min_size=0), lambda: g.frontiers(capacity=-1), lambda: g.frontiers(min_d2=-1)):
        with pytest.raises(solver.DirectError) as e:
            call()
        assert e.value.status == abi.DIRECT_ERR_INVALID
        assert np.array_equal(g.known_grid(), known) and np.array_equal(g.get_map(), grid)
    refused("no valid distance field", lambda: g.frontiers(min_d2=4))
    g.close()
