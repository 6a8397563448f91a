"""direct_cluster_map_from_cloud / direct_cluster_get_map (include/direct_cluster.h, "the map from a point cloud"; kernel in
direct_amd/csrc/map_cloud.h) on the device against the NumPy restatement of the reference's rcvPointCloudCallBack
(tests/map_cloud_harness.py, itself checked against the header program and the literal loop nest by
tests/test_map_cloud_restatement.py).  Maps are bytes and stats are counts: everything is compared for equality."""
import ctypes as C

import numpy as np
import pytest

from direct_amd import abi, cluster, problems
from tests import map_cloud_harness as mh

pytestmark = pytest.mark.gpu
BORDERS = (("clamp", mh.CLAMP), ("drop", mh.DROP))


@pytest.fixture(scope="module")
def gen(built):
    g = cluster.ClusterGenerator(mh.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)
    yield g
    g.close()


@pytest.fixture(scope="module")
def clouds():
    c = mh.clouds()
    rnd = c.pop("random")
    for n in (0, 1, 63, 64, 65, 1000):  # below, at and above one wave of lanes at margin 0; several workgroups at 1000
        c["random_%d" % n] = rnd[:n]
    return c


def stats_of(d):
    return [d["points"], d["skipped_nonfinite"], d["dropped"], d["occupied"]]


def from_cloud(gen, pts, margin, border, **kw):
    return gen.set_map_from_cloud(pts, mh.LOWER, mh.RES, margin, map_upper=mh.UPPER, border=border, **kw)


@pytest.mark.parametrize("margin", mh.MARGINS)
def test_map_and_stats_equal_the_restatement(gen, clouds, margin):
    for name, pts in clouds.items():
        for bname, border in BORDERS:
            want, wstats = mh.restate(pts, margin, border)
            st = from_cloud(gen, pts, margin, bname)
            got = gen.get_map()
            assert np.array_equal(got, want), (name, bname, int((got != want).sum()))
            assert stats_of(st) == wstats.tolist(), (name, bname, st, wstats)
    assert gen.last_ms() > 0.0


def test_a_box_larger_than_the_map(built):
    """9 x 7 x 5 voxels, margin 1.0: s = 7, s_z = 3, the box is 15 x 15 x 7 steps and every list is clamped or cut"""
    dims, lower = (9, 7, 5), np.array([0.3, -0.45, 0.15])
    upper = lower + np.array(dims) * mh.RES
    pts = np.concatenate([mh.cloud_random(40, dims, mh.RES, lower, seed=4), mh.cloud_borders(dims, mh.RES, lower, upper)])
    assert mh.steps(1.0, mh.RES) == (7, 3)
    g = cluster.ClusterGenerator(dims, max_batch=2, cluster_capacity=64, candidate_capacity=64)
    for bname, border in BORDERS:
        want, wstats = mh.restate(pts, 1.0, border, dims, mh.RES, lower, upper)
        st = g.set_map_from_cloud(pts, lower, mh.RES, 1.0, map_upper=upper, border=bname)
        assert np.array_equal(g.get_map(), want) and stats_of(st) == wstats.tolist(), (bname, st, wstats)
    # without map_upper the binding takes lower + dims * resolution
    assert stats_of(g.set_map_from_cloud(pts, lower, mh.RES, 1.0, border="drop")) == wstats.tolist()
    g.close()


def test_host_device_stride_and_order(gen):
    import torch
    pts = np.concatenate([mh.cloud_random(1000), mh.cloud_faces(), mh.cloud_borders(), mh.cloud_nonfinite()])
    for bname, border in BORDERS:
        want, wstats = mh.restate(pts, 0.25, border)
        for variant in (pts, mh.with_stride4(pts), pts[np.random.default_rng(3).permutation(len(pts))], pts[::-1]):
            for dev in (False, True):
                arg = torch.from_numpy(np.ascontiguousarray(variant)).to("cuda:0") if dev else variant
                st = from_cloud(gen, arg, 0.25, bname)
                assert np.array_equal(gen.get_map(), want), (bname, variant.shape, dev)
                assert stats_of(st) == wstats.tolist()
        out = torch.zeros(mh.DIMS, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert cluster._lib().direct_cluster_get_map(gen.h, abi.MEM_DEVICE, out.data_ptr()) == abi.DIRECT_OK
        assert np.array_equal(out.cpu().numpy(), want)


def test_add_and_replace(built):
    pts = mh.cloud_random(1000)
    whole, wstats = mh.restate(pts, 0.25, mh.CLAMP)
    g = cluster.ClusterGenerator(mh.DIMS, max_batch=2, cluster_capacity=64, candidate_capacity=64)
    # ADD on a handle without a map starts from an empty one
    st = from_cloud(g, pts[:500], 0.25, "clamp", add=True)
    half, hstats = mh.restate(pts[:500], 0.25, mh.CLAMP)
    assert np.array_equal(g.get_map(), half) and stats_of(st) == hstats.tolist()
    st = from_cloud(g, pts[500:], 0.25, "clamp", add=True)
    assert np.array_equal(g.get_map(), whole)
    assert stats_of(st) == [500, 0, 0, int(wstats[3])]
    # ADD of nothing changes nothing; REPLACE forgets the old points; REPLACE with nothing is an empty map, and it is a map
    assert from_cloud(g, pts[:0], 0.25, "clamp", add=True)["occupied"] == wstats[3] and np.array_equal(g.get_map(), whole)
    other, ostats = mh.restate(pts[:10], 0.0, mh.CLAMP)
    st = from_cloud(g, pts[:10], 0.0, "clamp")
    assert np.array_equal(g.get_map(), other) and stats_of(st) == ostats.tolist()
    assert stats_of(from_cloud(g, pts[:0], 0.25, "clamp")) == [0, 0, 0, 0] and not g.get_map().any()
    # ADD onto a map that set_map put there
    g.set_map(half)
    from_cloud(g, pts[500:], 0.25, "clamp", add=True)
    assert np.array_equal(g.get_map(), whole)
    g.close()


def same_results(a, b):
    for k in ("vertex_idx", "cluster_num", "iters", "rtn"):
        assert np.array_equal(a[0][k], b[0][k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a[0]["clusters"], b[0]["clusters"]))
    for k in ("path_len", "rtn"):
        assert np.array_equal(a[1][k], b[1][k]), k
    assert np.array_equal(a[1]["path_cost"].view(np.int64), b[1]["path_cost"].view(np.int64))
    assert all(np.array_equal(x, y) for x, y in zip(a[1]["paths"], b[1]["paths"]))


def test_the_summed_area_table_is_rebuilt(built):
    """polygon_generation (whose convex tests read the summed-area table) and grid_paths after set_map_from_cloud equal those
    after set_map(the restatement's map) on a second handle; again after an ADD that closes the map across x, which a table left
    over from the first map would not know"""
    dims, res, lower = (60, 56, 16), 0.15, np.array([-4.5, -4.2, 0.0])
    upper = lower + np.array(dims) * res
    pts = problems.make_point_cloud(dims, res, lower, seed=5)
    m1, s1 = mh.restate(pts, 0.25, mh.CLAMP, dims, res, lower, upper)
    y, z = np.meshgrid(np.arange(dims[1]), np.arange(dims[2]), indexing="ij")
    wall = (lower + (np.stack([np.full(y.size, 30), y.ravel(), z.ravel()], axis=1) + 0.5) * res).astype(np.float32)
    m2, s2 = mh.restate(wall, 0.0, mh.CLAMP, dims, res, lower, upper, base=m1)
    assert m2[30].all() and not m1[30].all()
    free = np.argwhere(m2 == 0)
    rng = np.random.default_rng(6)
    near = free[np.abs(free[:, 0] - 30) <= 3]
    seeds = np.concatenate([near[rng.choice(len(near), 8, replace=False)], free[rng.choice(len(free), 8, replace=False)]]).astype(np.int32)
    left, right = free[free[:, 0] < 30], free[free[:, 0] > 30]
    starts = left[rng.choice(len(left), 8, replace=False)].astype(np.int32)
    goals = np.concatenate([right[rng.choice(len(right), 4, replace=False)], left[rng.choice(len(left), 4, replace=False)]]).astype(np.int32)
    a = cluster.ClusterGenerator(dims, max_batch=16)
    b = cluster.ClusterGenerator(dims, max_batch=16)
    run = lambda g: (g.polygon_generation(seeds), g.grid_paths(starts, goals))
    st = a.set_map_from_cloud(pts, lower, res, 0.25, map_upper=upper)
    assert stats_of(st) == s1.tolist() and np.array_equal(a.get_map(), m1)
    b.set_map(m1)
    ra1, rb1 = run(a), run(b)
    same_results(ra1, rb1)
    st = a.set_map_from_cloud(wall, lower, res, 0.0, map_upper=upper, add=True)
    assert stats_of(st) == s2.tolist() and np.array_equal(a.get_map(), m2)
    b.set_map(m2)
    ra2, rb2 = run(a), run(b)
    same_results(ra2, rb2)
    a.close()
    b.close()
    # the cases can tell the two maps apart: the wall cuts the crossing paths, and some cluster changes
    assert (ra1[1]["rtn"][:4] == cluster.GRID_PATH_OK).all() and (ra2[1]["rtn"][:4] == cluster.GRID_PATH_NO_PATH).all()
    assert (ra1[0]["rtn"] == cluster.CLUSTER_OK).all() and (ra2[0]["rtn"] == cluster.CLUSTER_OK).all()
    assert any(not np.array_equal(x, y) for x, y in zip(ra1[0]["clusters"], ra2[0]["clusters"]))


def test_error_returns(built):
    L = cluster._lib()
    g = cluster.ClusterGenerator(mh.DIMS, max_batch=2, cluster_capacity=64, candidate_capacity=64)
    pts = mh.cloud_random(8)
    grid = np.zeros(mh.DIMS, np.uint8)
    assert L.direct_cluster_get_map(g.h, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_ERR_INVALID  # no map yet

    def call(h=None, par=True, n=8, mem=abi.MEM_HOST, xyz=True, **field):
        v = dict(resolution=mh.RES, cloud_margin=0.25, border=cluster.MAP_BORDER_CLAMP, mode=cluster.MAP_REPLACE, stride=3)
        v.update(field)
        p = cluster.MapCloud((C.c_double * 3)(*mh.LOWER), (C.c_double * 3)(*mh.UPPER), v["resolution"], v["cloud_margin"], v["border"],
                             v["mode"], v["stride"], 0)
        return L.direct_cluster_map_from_cloud(g.h if h is None else h, C.addressof(p) if par else None, n, mem,
                                               pts.ctypes.data if xyz else None, None)

    bad = [dict(h=C.c_void_p()), dict(par=False), dict(n=-1), dict(xyz=False), dict(resolution=0.0), dict(resolution=-0.15),
           dict(resolution=float("nan")), dict(resolution=float("inf")), dict(cloud_margin=-0.01), dict(cloud_margin=float("nan")),
           dict(cloud_margin=float("inf")), dict(stride=2), dict(stride=5), dict(border=2), dict(border=-1), dict(mode=2), dict(mode=-1),
           dict(mem=7)]
    for kw in bad:
        assert call(**kw) == abi.DIRECT_ERR_INVALID, kw
        assert len(L.direct_cluster_last_error()) > 0
    assert L.direct_cluster_get_map(g.h, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_ERR_INVALID  # a refused call makes no map
    assert call(cloud_margin=200.0) == abi.DIRECT_ERR_UNSUPPORTED
    assert call(n=0, xyz=False) == abi.DIRECT_OK                 # no points need no pointer: an empty map
    assert L.direct_cluster_get_map(g.h, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_OK and not grid.any()
    assert L.direct_cluster_get_map(g.h, abi.MEM_HOST, None) == abi.DIRECT_ERR_INVALID
    assert L.direct_cluster_get_map(None, abi.MEM_HOST, grid.ctypes.data) == abi.DIRECT_ERR_INVALID
    assert call() == abi.DIRECT_OK                               # stats may be NULL
    assert np.array_equal(g.get_map(), mh.restate(pts, 0.25, mh.CLAMP)[0])
    g.close()
