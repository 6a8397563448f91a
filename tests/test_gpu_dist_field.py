"""direct_cluster_distance_field on the GPU against the NumPy brute force of tests/dist_field_harness.py: the stored field integer
for integer, its stats, its staleness after every call that touches the map, and that the other stages do not notice it."""
import ctypes as C

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import dist_field_harness as dh
from tests import map_cloud_harness as mh
from tests import plan_check_harness as ph

pytestmark = pytest.mark.gpu


def small(dims):
    return cluster.ClusterGenerator(dims, max_batch=4, cluster_capacity=2048, candidate_capacity=512)


@pytest.fixture(scope="module")
def exact():
    """name -> (grid, uncapped brute force), once"""
    return {name: (g, dh.brute_d2(g)) for name, g in dh.shared_grids()}


@pytest.mark.parametrize("shape", [(40, 36, 12)] + list(dh.SHAPES))
def test_field_equals_brute_force(built, exact, shape):
    import torch
    names = ["shared_map"] if shape == (40, 36, 12) else ["%dx%dx%d %s" % (tuple(shape) + (d,)) for d in dh.DENSITIES]
    g = small(shape)
    for name in names:
        grid, d2 = exact[name]
        g.set_map(grid)
        for cap in (0, 4):
            want = np.minimum(d2, dh.cap2_of(cap)).astype(np.int32)
            stats = g.build_distance_field(cap)
            got = g.distance_field()
            bad = np.argwhere(got != want)
            assert not len(bad), f"{name} cap {cap}: {len(bad)} voxels differ, first {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
            assert stats == dh.field_stats(want, cap), f"{name} cap {cap}"
            assert g.last_ms() > 0.0
        dev = g.distance_field(out=torch.full(shape, -5, dtype=torch.int32, device="cuda:0"))
        assert np.array_equal(dev.cpu().numpy(), want), name
    g.close()


def clearance_code(g, inp):
    """the status code of the clearance call on a valid input, and its status array prefilled with 77"""
    T, coef, n_seg = (np.ascontiguousarray(inp["T"], np.float64), np.ascontiguousarray(inp["bez"], np.float64),
                      np.ascontiguousarray(inp["n_seg"], np.int32))
    B, N = T.shape
    par = cluster.PlanClearIn(batch=B, n_seg_max=N, mem=abi.MEM_HOST, dtype=abi.F64, n_seg=n_seg.ctypes.data, T=T.ctypes.data,
                              bez=coef.ctypes.data, map_lower=(C.c_double * 3)(*ph.LOWER), resolution=ph.RES, radius=0.2, depth=3)
    status = np.full(B, 77, np.int32)
    o = cluster.PlanClearOut(status=status.ctypes.data)
    return cluster._lib().direct_cluster_plan_clearance_batch(g.h, C.addressof(par), C.addressof(o)), status


def fetch_code(g):
    d2 = np.full(g.dims, 77, np.int32)
    return cluster._lib().direct_cluster_get_distance_field(g.h, abi.MEM_HOST, d2.ctypes.data), d2


def assert_stale(g, inp):
    st, status = clearance_code(g, inp)
    assert st == abi.DIRECT_ERR_INVALID and (status == 77).all() and b"distance field" in cluster._lib().direct_cluster_last_error()
    st, d2 = fetch_code(g)
    assert st == abi.DIRECT_ERR_INVALID and (d2 == 77).all()


def test_staleness(built):
    grid = ph.shared_map()
    inp = ph.pick(ph.random7(), "bez")
    g = small(mh.DIMS)
    g.set_map(grid)
    assert_stale(g, inp)                                  # before any build
    g.build_distance_field()
    assert clearance_code(g, inp)[0] == abi.DIRECT_OK and fetch_code(g)[0] == abi.DIRECT_OK
    g.set_map(grid)
    assert_stale(g, inp)                                  # after set_map, even of the same map
    g.build_distance_field(4)
    assert np.array_equal(g.distance_field(), dh.brute_d2(grid, 4))
    point = np.array([[-1.7, ph.lane_y(0), ph.LANE_Z]], np.float32)
    g.set_map_from_cloud(point, ph.LOWER, ph.RES, cloud_margin=0.0, add=True)
    assert_stale(g, inp)                                  # after a cloud was added
    merged = g.get_map()
    assert merged.sum() > grid.sum()
    g.build_distance_field()
    assert np.array_equal(g.distance_field(), dh.brute_d2(merged))
    with pytest.raises(solver.DirectError):               # a cloud call that fails its argument check marks the field stale too
        g.set_map_from_cloud(point, ph.LOWER, -1.0, add=True)
    assert_stale(g, inp)
    g.close()


def test_other_stages_are_untouched(built):
    """a grid path and a plan check before and after a build are identical: the field shares no workspace with them"""
    grid = ph.shared_map()
    inp = ph.pick(ph.long5(), "poly")
    g = small(mh.DIMS)
    g.set_map(grid)
    free = np.argwhere(grid[:20] == 0)
    ends = free[np.random.default_rng(7).choice(len(free), 4, replace=False)].astype(np.int32)

    def both():
        p = g.grid_paths(ends[:2], ends[2:])
        c = g.check_plans(inp["n_seg"], inp["T"], ph.LOWER, ph.RES, poly=inp["poly"], depth=7, t_from=inp["t_from"])
        return p, c
    p0, c0 = both()
    g.build_distance_field()
    g.plan_clearance(inp["n_seg"], inp["T"], ph.LOWER, ph.RES, poly=inp["poly"], depth=7, t_from=inp["t_from"])
    p1, c1 = both()
    assert np.array_equal(p0["rtn"], p1["rtn"]) and np.array_equal(p0["path_len"], p1["path_len"])
    assert all(np.array_equal(x, y) for x, y in zip(p0["paths"], p1["paths"]))
    assert np.array_equal(p0["path_cost"].view(np.int64), p1["path_cost"].view(np.int64))
    ph.assert_same(c1, c0, "check_plans after a build")
    assert np.array_equal(g.distance_field(), dh.brute_d2(grid))     # and they left the field alone
    g.close()


def test_invalid_arguments_launch_nothing(built):
    lib = cluster._lib()
    g = small((5, 4, 3))
    stats = np.full(2, 77, np.int64)
    assert lib.direct_cluster_distance_field(g.h, 0, stats.ctypes.data) == abi.DIRECT_ERR_INVALID     # no map
    assert b"map" in lib.direct_cluster_last_error() and (stats == 77).all()
    d2 = np.full((5, 4, 3), 77, np.int32)
    assert lib.direct_cluster_get_distance_field(g.h, abi.MEM_HOST, d2.ctypes.data) == abi.DIRECT_ERR_INVALID
    g.set_map(np.zeros((5, 4, 3), np.uint8))
    assert lib.direct_cluster_distance_field(None, 0, stats.ctypes.data) == abi.DIRECT_ERR_INVALID
    for cap in (-1, 1025):
        assert lib.direct_cluster_distance_field(g.h, cap, stats.ctypes.data) == abi.DIRECT_ERR_INVALID
    assert (stats == 77).all()
    assert lib.direct_cluster_get_distance_field(g.h, abi.MEM_HOST, d2.ctypes.data) == abi.DIRECT_ERR_INVALID   # the failed builds built nothing
    assert lib.direct_cluster_distance_field(g.h, 1024, None) == abi.DIRECT_OK                    # stats may be NULL
    assert lib.direct_cluster_get_distance_field(None, abi.MEM_HOST, d2.ctypes.data) == abi.DIRECT_ERR_INVALID
    assert lib.direct_cluster_get_distance_field(g.h, 2, d2.ctypes.data) == abi.DIRECT_ERR_INVALID
    assert lib.direct_cluster_get_distance_field(g.h, abi.MEM_HOST, None) == abi.DIRECT_ERR_INVALID
    assert (d2 == 77).all()
    assert lib.direct_cluster_get_distance_field(g.h, abi.MEM_HOST, d2.ctypes.data) == abi.DIRECT_OK and (d2 == 1024 * 1024).all()
    assert g.build_distance_field() == dict(below_cap=0, max_d2=-1) and (g.distance_field() == cluster.DIST_NONE).all()
    g.close()
