"""direct_cluster_map_integrate_scan / direct_cluster_get_scan_grid (include/direct_cluster.h, "one sensor scan folded into the
map"; kernels in direct_amd/csrc/map_scan.h) on the device against the restatement in Python floats and the g++ build of the same
header (tests/map_scan_harness.py, themselves held equal by tests/test_map_scan_restatement.py).  Grids are bytes and stats are
counts: everything is compared for equality."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh
from tests import plan_check_harness as ph

pytestmark = pytest.mark.gpu
ROOT = sh.ROOT
SMALL = dict(max_batch=4, cluster_capacity=64, candidate_capacity=64)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("map_scan_gpu"))


@pytest.fixture(scope="module")
def gen(built):
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    yield g
    g.close()


def stats_of(d):
    return [d[k] for k in sh.STATS]


def scan(g, pts, max_range, inflate=(0, 0, 0), mode="continue", origin=sh.ORIGIN, **kw):
    return g.integrate_scan(pts, origin, sh.LOWER, sh.RES, max_range, inflate=inflate, mode=mode, map_upper=sh.UPPER, **kw)


def check(g, st, want, what):
    raw, new, wstats = want
    got_raw, got_map = g.scan_grid(), g.get_map()
    assert np.array_equal(got_raw, raw), (what, "raw", int((got_raw != raw).sum()))
    assert np.array_equal(got_map, new), (what, "map", int((got_map != new).sum()))
    assert stats_of(st) == wstats.tolist(), (what, st, wstats)


@pytest.mark.parametrize("inflate", ((0, 0, 0), (2, 2, 1)))
def test_grids_and_stats_equal_the_restatement(gen, inflate):
    """n below, at and above one wave and several workgroups; every cloud of the CPU tests at the three ranges; on an empty scan
    grid (RESET) and, for the random cloud, on a full one (ADOPT of a map of ones), where the carve is what shows"""
    clouds = sh.clouds()
    rnd = clouds.pop("random")
    for n in (0, 1, 63, 64, 65, 1000):
        clouds["random_%d" % n] = rnd[:n]
    full = np.ones(sh.DIMS, np.uint8)
    gen.set_map(full)
    for name, pts in clouds.items():
        for r in sh.RANGES if name in ("random_1000", "lattice") else (1.5,):
            before = gen.get_map()
            check(gen, scan(gen, pts, r, inflate, "reset"), sh.restate(pts, sh.ORIGIN, r, inflate, before=before), (name, r, "reset"))
            if name.startswith("random"):
                gen.set_map(full)
                check(gen, scan(gen, pts, r, inflate, "adopt"), sh.restate(pts, sh.ORIGIN, r, inflate, raw=full, before=full), (name, r, "adopt"))
    assert gen.last_ms() > 0.0


def test_the_three_modes_in_sequence(built):
    pts = mh.cloud_random(1000)
    a, b, c = pts[:400], pts[400:700], pts[700:]
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    with pytest.raises(solver.DirectError):
        g.scan_grid()                                                    # no scan grid yet
    # CONTINUE on a handle without a scan grid (and without a map) starts empty
    w1 = sh.restate(a, sh.ORIGIN, 10.0, (2, 2, 1))
    check(g, scan(g, a, 10.0, (2, 2, 1)), w1, "continue on nothing")
    w2 = sh.restate(b, sh.ORIGIN, 10.0, (2, 2, 1), raw=w1[0], before=w1[1])
    check(g, scan(g, b, 10.0, (2, 2, 1)), w2, "continue")
    assert w2[2][6] > 0 and w2[2][7] > 0
    # the scan grid outlives a set_map; CONTINUE ignores the map's bytes but counts the changes against them
    other = ph.shared_map()
    g.set_map(other)
    w3 = sh.restate(c, sh.ORIGIN, 1.5, (0, 0, 0), raw=w2[0], before=other)
    check(g, scan(g, c, 1.5), w3, "continue after set_map")
    # ADOPT takes the map that set_map or map_from_cloud left
    g.set_map(other)
    w4 = sh.restate(a, sh.ORIGIN, 1.5, (1, 0, 2), raw=other, before=other)
    check(g, scan(g, a, 1.5, (1, 0, 2), "adopt"), w4, "adopt after set_map")
    g.set_map_from_cloud(b, sh.LOWER, sh.RES, 0.25, map_upper=sh.UPPER)
    added = g.get_map()
    w5 = sh.restate(c, sh.ORIGIN, 10.0, raw=added, before=added)
    check(g, scan(g, c, 10.0, mode="adopt"), w5, "adopt after map_from_cloud")
    assert w5[2][7] > 0
    # RESET forgets; RESET with no points is an empty map, and it is a map
    w6 = sh.restate(b, sh.ORIGIN, 10.0, before=w5[1])
    check(g, scan(g, b, 10.0, mode="reset"), w6, "reset")
    st = scan(g, b[:0], 10.0, mode="reset")
    assert stats_of(st) == [0, 0, 0, 0, 0, 0, 0, int(w6[1].sum())] and not g.get_map().any() and not g.scan_grid().any()
    g.close()


def test_a_box_larger_than_the_map(built):
    """9 x 7 x 5 voxels, inflate (15, 15, 7) and the limit (64, 64, 64): every list is cut at the border"""
    dims, lower = (9, 7, 5), np.array([0.3, -0.45, 0.15])
    upper = lower + np.array(dims) * sh.RES
    origin = lower + np.array([4.3, 3.6, 2.2]) * sh.RES
    pts = np.concatenate([mh.cloud_random(40, dims, sh.RES, lower, seed=4), mh.cloud_borders(dims, sh.RES, lower, upper)])
    one = (lower + (np.array([[8, 0, 4]]) + 0.5) * sh.RES).astype(np.float32)
    g = cluster.ClusterGenerator(dims, **SMALL)
    g.set_map(np.zeros(dims, np.uint8))
    for cloud in (pts, one, one[:0]):
        for inflate in ((15, 15, 7), (64, 64, 64), (1, 0, 0), (0, 3, 0), (0, 0, 2)):
            want = sh.restate(cloud, origin, 1.0, inflate, before=g.get_map(), dims=dims, lower=lower, upper=upper)
            st = g.integrate_scan(cloud, origin, lower, sh.RES, 1.0, inflate=inflate, mode="reset")   # map_upper: lower + dims * res
            check(g, st, want, (len(cloud), inflate))
            assert len(cloud) == 0 or inflate[0] < 15 or want[1].all()
    g.close()


def test_the_grid_stride_loops_take_a_second_trip(built, exe):
    """300 000 rays (1024 workgroups of 256 lanes hold 262 144) on a full scan grid, against the g++ build of the header: the Python
    restatement would take too long.  The points lie 1.2 to 2.5 m from the origin in every direction and max_range is 1.5 m: hits
    inside and outside the map, truncated rays, and a carved ball that outlives the dilation."""
    rng = np.random.default_rng(9)
    d = rng.normal(0.0, 1.0, (300000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = (sh.ORIGIN + d * rng.uniform(1.2, 2.5, (300000, 1))).astype(np.float32)
    pts[::1000, 1] = np.nan
    full = np.ones(sh.DIMS, np.uint8)
    raw, new, wstats, _ = sh.run(exe, pts, sh.ORIGIN, 1.5, (2, 2, 1), raw=full, before=full)
    assert wstats[1] == 300 and wstats[2] > 50000 and wstats[3] > 10000 and wstats[0] - wstats[1] - wstats[2] > 50000 and wstats[7] > 100
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    g.set_map(full)
    check(g, scan(g, pts, 1.5, (2, 2, 1), "adopt"), (raw, new, wstats), "300000 rays")
    g.close()


def test_host_device_stride_and_order(gen):
    import torch
    pts = np.concatenate(list(sh.clouds().values()))
    full = np.ones(sh.DIMS, np.uint8)
    want = sh.restate(pts, sh.ORIGIN, 1.5, (2, 2, 1), raw=full, before=full)
    for variant in (pts, mh.with_stride4(pts), pts[np.random.default_rng(3).permutation(len(pts))], pts[::-1]):
        for dev in (False, True):
            arg = torch.from_numpy(np.ascontiguousarray(variant)).to("cuda:0") if dev else variant
            gen.set_map(full)
            check(gen, scan(gen, arg, 1.5, (2, 2, 1), "adopt"), want, (variant.shape, dev))
    out = torch.zeros(sh.DIMS, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert cluster._lib().direct_cluster_get_scan_grid(gen.h, abi.MEM_DEVICE, out.data_ptr()) == abi.DIRECT_OK
    assert np.array_equal(out.cpu().numpy(), want[0])


def test_a_wall_seen_through_leaves_the_map(built):
    """the scenario of the CPU tests on the device, the ADDed wall included"""
    wpts, room, wall = sh.wall_and_room()
    w = tuple(wall.T)
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    s1 = scan(g, wpts, 10.0, (2, 2, 1))
    shell = g.get_map() == 1
    assert g.scan_grid()[w].all() and s1["raw_occupied"] == len(wall) and s1["set"] == shell.sum() > 3 * len(wall)
    s2 = scan(g, room, 10.0, (2, 2, 1))
    assert not g.scan_grid()[w].any() and not g.get_map()[shell].any() and s2["cleared"] == shell.sum()
    s3 = scan(g, room, 10.0, (2, 2, 1))
    assert s3["set"] == 0 and s3["cleared"] == 0 and s3["occupied"] == s2["occupied"]
    g.set_map_from_cloud(wpts, sh.LOWER, sh.RES, 0.0, map_upper=sh.UPPER)
    g.set_map_from_cloud(room, sh.LOWER, sh.RES, 0.0, map_upper=sh.UPPER, add=True)
    added = g.get_map()
    assert added[w].all()                                                # ADD keeps the wall for ever
    s4 = scan(g, room, 10.0, mode="adopt")
    assert not g.get_map()[w].any() and s4["cleared"] > len(wall)
    g.close()


def test_the_tables_follow_the_map(built):
    """after a scan, a second handle given set_map(get_map()) returns the same check_plans and polygon_generation outputs: the
    summed-area table was rebuilt from the map the scan left"""
    pts = mh.cloud_random(1000)
    inp = ph.pick(ph.long5(), "poly")
    a = cluster.ClusterGenerator(sh.DIMS, max_batch=16)
    b = cluster.ClusterGenerator(sh.DIMS, max_batch=16)
    a.set_map(ph.shared_map())
    a.polygon_generation(np.array([[22, 16, 6]], np.int32))              # tables of the old map are in use
    for k, (cloud, mode) in enumerate(((pts[:600], "adopt"), (pts[600:], "continue"))):
        st = scan(a, cloud, 1.5, (1, 1, 0), mode)
        assert st["set"] + st["cleared"] > 0
        grid = a.get_map()
        b.set_map(grid)
        free = np.argwhere(grid == 0)
        seeds = free[np.random.default_rng(20 + k).choice(len(free), 12, replace=False)].astype(np.int32)
        ra, rb = a.polygon_generation(seeds), b.polygon_generation(seeds)
        for key in ("vertex_idx", "cluster_num", "iters", "rtn"):
            assert np.array_equal(ra[key], rb[key]), key
        assert all(np.array_equal(x, y) for x, y in zip(ra["clusters"], rb["clusters"]))
        assert (ra["rtn"] == cluster.CLUSTER_OK).any() and (ra["cluster_num"] > 1).any()
        ca, cb = (g.check_plans(inp["n_seg"], inp["T"], ph.LOWER, ph.RES, poly=inp["poly"], depth=7, t_from=inp["t_from"]) for g in (a, b))
        ph.assert_same(ca, cb, "check_plans after a scan")
    a.close()
    b.close()


def test_staleness_follows_the_change_counts(built):
    """plan_clearance and reachable refuse as stale after a scan that changed the map, and still serve, with the same bytes, after
    a scan with set + cleared == 0"""
    pts = mh.cloud_random(600)
    inp = ph.pick(ph.random7(), "poly")
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    scan(g, pts[:300], 10.0, (1, 1, 1), "reset")
    grid = g.get_map()
    free = np.argwhere(grid == 0)
    ends = free[np.random.default_rng(5).choice(len(free), 8, replace=False)].astype(np.int32)

    def serve():
        c = g.plan_clearance(inp["n_seg"], inp["T"], ph.LOWER, ph.RES, poly=inp["poly"], depth=5, t_from=inp["t_from"])
        r = g.reachable(ends[:4], ends[4:], min_d2=2)
        return [np.asarray(v).tobytes() for v in c.values()] + [np.asarray(v).tobytes() for v in r]

    def stale(word, call):
        with pytest.raises(solver.DirectError) as e:
            call()
        assert e.value.status == abi.DIRECT_ERR_INVALID and word in str(e.value), str(e.value)

    clear = lambda: g.plan_clearance(inp["n_seg"], inp["T"], ph.LOWER, ph.RES, poly=inp["poly"], depth=5, t_from=inp["t_from"])
    reach = lambda: g.reachable(ends[:4], ends[4:], min_d2=2)
    stale("no valid distance field", clear)                              # a first scan made a map: nothing describes it yet
    g.build_distance_field()
    g.build_free_components(2)
    first = serve()
    field = g.distance_field().tobytes()
    for mode in ("continue", "continue", "adopt"):                       # the same scan again, and the map adopted: nothing changes
        st = scan(g, pts[:300], 10.0, (1, 1, 1), mode) if mode == "continue" else scan(g, pts[:0], 10.0, (0, 0, 0), mode)
        assert st["set"] + st["cleared"] == 0 and np.array_equal(g.get_map(), grid)
        assert serve() == first and g.distance_field().tobytes() == field
    st = scan(g, pts[300:], 10.0, (1, 1, 1))
    assert st["set"] + st["cleared"] > 0
    stale("no valid distance field", clear)
    stale("no valid", reach)
    g.build_distance_field()
    stale("no valid free components", reach)
    g.build_free_components(2)
    assert serve() != first
    # a refused call leaves everything as it was
    with pytest.raises(solver.DirectError):
        scan(g, pts, -1.0)
    serve()
    g.close()


def test_error_returns(built):
    L = cluster._lib()
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    pts = mh.cloud_random(8)
    grid = np.zeros(sh.DIMS, np.uint8)
    assert L.direct_cluster_get_scan_grid(g.h, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_ERR_INVALID   # no scan grid yet

    def call(h=None, par=True, n=8, mem=abi.MEM_HOST, xyz=True, lower=sh.LOWER, upper=sh.UPPER, origin=sh.ORIGIN, inflate=(0, 0, 0), **field):
        v = dict(resolution=sh.RES, max_range=1.5, mode=cluster.SCAN_CONTINUE, stride=3)
        v.update(field)
        p = cluster.MapScan((C.c_double * 3)(*lower), (C.c_double * 3)(*upper), v["resolution"], v["max_range"], (C.c_double * 3)(*origin),
                            (C.c_int32 * 3)(*inflate), v["mode"], v["stride"], 0)
        return L.direct_cluster_map_integrate_scan(g.h if h is None else h, C.addressof(p) if par else None, n, mem,
                                                   pts.ctypes.data if xyz else None, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(h=C.c_void_p()), dict(par=False), dict(n=-1), dict(xyz=False), dict(mem=7), dict(mode=3), dict(mode=-1), dict(stride=2),
           dict(stride=5), dict(resolution=0.0), dict(resolution=-0.15), dict(resolution=nan), dict(resolution=inf), dict(max_range=0.0),
           dict(max_range=-1.0), dict(max_range=nan), dict(max_range=inf), dict(lower=(nan, -2.7, 0.0)), dict(upper=(3.0, inf, 1.85)),
           dict(origin=(-3.01, 0.0, 0.5)), dict(origin=(3.0, 0.0, 0.5)), dict(origin=(0.0, 0.0, 1.82)), dict(origin=(0.0, nan, 0.5)),
           dict(inflate=(0, -1, 0)), dict(mode=cluster.SCAN_ADOPT)]
    for kw in bad:
        assert call(**kw) == abi.DIRECT_ERR_INVALID, kw
        assert len(L.direct_cluster_last_error()) > 0
    assert L.direct_cluster_get_map(g.h, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_ERR_INVALID        # a refused call makes no map
    assert L.direct_cluster_get_scan_grid(g.h, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_ERR_INVALID  # ... and no scan grid
    assert call(max_range=4096.5 * sh.RES) == abi.DIRECT_ERR_UNSUPPORTED
    assert call(inflate=(0, 0, 65)) == abi.DIRECT_ERR_UNSUPPORTED
    assert call(max_range=4095 * sh.RES, inflate=(64, 64, 64), n=0, xyz=False) == abi.DIRECT_OK   # the limits; no points need no pointer
    assert L.direct_cluster_get_map(g.h, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_OK and not grid.any()
    assert call(mode=cluster.SCAN_ADOPT) == abi.DIRECT_OK                                          # now there is a map to adopt
    assert L.direct_cluster_get_scan_grid(g.h, abi.MEM_HOST, None) == abi.DIRECT_ERR_INVALID
    assert L.direct_cluster_get_scan_grid(None, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_ERR_INVALID
    assert L.direct_cluster_get_scan_grid(g.h, 7, grid.ctypes.data) == abi.DIRECT_ERR_INVALID
    assert call() == abi.DIRECT_OK                                                                 # stats may be NULL
    assert L.direct_cluster_get_scan_grid(g.h, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_OK
    assert np.array_equal(grid, sh.restate(pts, sh.ORIGIN, 1.5)[0])
    ms = (C.c_float * 4)()
    assert L.direct_cluster_scan_phase_ms(g.h, ms) == abi.DIRECT_ERR_INVALID                       # the handle records no phases
    g.close()


def test_cpp_mirror_against_the_python_call(built, tmp_path):
    """polyhedronGenerator::integrateScan / getMap (direct_amd/host/poly_utils.hpp) give the binding's stats and maps for a sequence
    of scans in the three modes (tests/cpp/test_map_scan_gen.cpp)"""
    pts = mh.cloud_random(900)
    start = ph.shared_map()
    fin, exe = str(tmp_path / "in.bin"), str(tmp_path / "gen")
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    g.set_map(start)
    scans = ((cluster.SCAN_ADOPT, "adopt", (0, 0, 0), pts[:300]), (cluster.SCAN_CONTINUE, "continue", (2, 2, 1), pts[300:600]),
             (cluster.SCAN_CONTINUE, "continue", (2, 2, 1), pts[300:600]), (cluster.SCAN_RESET, "reset", (1, 0, 0), pts[600:]))
    with open(fin, "wb") as f:
        f.write(struct.pack("<3id3d3dd", *sh.DIMS, sh.RES, *sh.LOWER, *sh.ORIGIN, 1.5))
        f.write(start.tobytes())
        f.write(struct.pack("<i", len(scans)))
        for code, mode, inflate, cloud in scans:
            st = g.integrate_scan(cloud, sh.ORIGIN, sh.LOWER, sh.RES, 1.5, inflate=inflate, mode=mode)
            f.write(struct.pack("<5i", code, *inflate, len(cloud)))
            f.write(np.ascontiguousarray(cloud, np.float32).tobytes())
            f.write(np.array(stats_of(st), np.int64).tobytes() + g.get_map().tobytes())
    g.close()
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests/cpp/test_map_scan_gen.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "direct_amd/lib"), "-ldirect_ddp",
                           "-Wl,-rpath," + os.path.join(ROOT, "direct_amd/lib") + ":/opt/rocm/lib"])
    out = subprocess.run([exe, fin], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
