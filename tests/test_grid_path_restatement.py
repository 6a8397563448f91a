"""Grid paths (include/direct_cluster.h, "grid paths") on the CPU: direct_amd/csrc/grid_path_math.h compiled by g++
(tests/grid_path_harness.py).  1. an independent witness - a heapq Dijkstra and the predecessor rule written here, not via the
header - against the harness's Dijkstra, bit for bit; 2. the emulated tiled relaxation against that Dijkstra on the
200 x 200 x 40 map, and every return code; 3. properties of the returned paths that need no oracle."""
import heapq
import math
import os

import numpy as np
import pytest

from tests import grid_path_harness as gh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = {1: 1.0, 2: math.sqrt(2.0), 3: math.sqrt(3.0)}
NB = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return gh.build(tmp_path_factory.mktemp("grid_path"))


def witness(grid, start, goal):
    """-> (field, path or None): Dijkstra from `start` over the 26-neighbourhood into free voxels, one float addition per move;
    the path by the contract's predecessor rule"""
    X, Y, Z = grid.shape
    d = np.full(grid.shape, np.inf)
    d[tuple(start)] = 0.0
    heap = [(0.0, tuple(int(v) for v in start))]
    while heap:
        dv, v = heapq.heappop(heap)
        if dv != d[v]:
            continue
        for o in NB:
            u = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if not (0 <= u[0] < X and 0 <= u[1] < Y and 0 <= u[2] < Z) or grid[u] != 0:
                continue
            c = dv + W[abs(o[0]) + abs(o[1]) + abs(o[2])]
            if c < d[u]:
                d[u] = c
                heapq.heappush(heap, (c, u))
    v = tuple(int(c) for c in goal)
    if not np.isfinite(d[v]):
        return d, None
    path = [v]
    while v != tuple(int(c) for c in start):
        for o in NB:  # ascending (dx, dy, dz)
            u = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if 0 <= u[0] < X and 0 <= u[1] < Y and 0 <= u[2] < Z and d[u] + W[abs(o[0]) + abs(o[1]) + abs(o[2])] == d[v]:
                v = u
                break
        else:
            raise AssertionError("no predecessor")
        path.append(v)
    return d, np.array(path[::-1], np.int32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def test_header_and_export_exist():
    from direct_amd import cluster
    assert "direct_cluster_grid_path_batch" in cluster.EXPORTS
    text = open(os.path.join(ROOT, "include", "direct_cluster.h")).read()
    for name in ("NO_PATH", "BAD_ENDPOINT", "OVERFLOW", "ROUND_LIMIT"):
        assert "DIRECT_GRID_PATH_" + name in text
    assert os.path.exists(os.path.join(ROOT, "direct_amd", "csrc", "grid_path_math.h"))


@pytest.mark.parametrize("name", ["partial_tiles", "sealed_box", "flat", "maze", "tile_serpentine"])
def test_witness_small_maps(harness, name):
    """1.  maps up to 32 x 24 x 12: a 2-D map, dims that are no multiples of 8, a sealed box, a serpentine maze"""
    case = next(c for c in gh.crafted_cases() if c["name"] == name)
    grid = case["grid"]
    assert grid.shape[0] <= 32 and grid.shape[1] <= 24 and grid.shape[2] <= 12
    X, Y, Z = grid.shape
    keep = [q for q in range(len(case["starts"])) if all(0 <= case[k][q][a] < grid.shape[a] for k in ("starts", "goals") for a in range(3))]
    starts, goals = case["starts"][keep], case["goals"][keep]
    r = gh.run(harness, grid, starts, goals, 4096, 0, sides=("full", "emu"))
    for q in range(len(keep)):
        d, path = witness(grid, starts[q], goals[q])
        assert same_bits(r["full"]["dist"][q], d.ravel()), (name, q)
        for side in ("full", "emu"):
            o = r[side]
            if path is None:
                assert o["rtn"][q] == gh.NO_PATH and o["path_len"][q] == 0 and np.isposinf(o["path_cost"][q])
                assert same_bits(o["dist"][q], d.ravel())  # the whole component, and +inf outside it
            else:
                assert o["rtn"][q] == gh.OK and o["path_len"][q] == len(path)
                assert same_bits(o["path_cost"][q], d[tuple(goals[q])])
                assert np.array_equal(o["paths"][q], path), (name, side, q)


@pytest.fixture(scope="module")
def big(harness):
    grid = gh.big_map()
    starts, goals = gh.big_queries(grid, 8)
    return grid, starts, goals, gh.run(harness, grid, starts, goals, 4096, 0, sides=("full", "emu"))


def test_emulated_rounds_big_map(big):
    """2.  8 queries with |delta|_1 > 120 on the 200 x 200 x 40 map: the tiled relaxation with the pruning bound against the heap"""
    grid, starts, goals, r = big
    full, emu = r["full"], r["emu"]
    for q in range(len(starts)):
        assert full["rtn"][q] == gh.OK and emu["rtn"][q] == gh.OK
        cost = full["path_cost"][q]
        assert same_bits(emu["path_cost"][q], cost)
        assert emu["path_len"][q] == full["path_len"][q] and np.array_equal(emu["paths"][q], full["paths"][q])
        true, got = full["dist"][q], emu["dist"][q]
        near = true <= cost
        assert near.sum() > 1000
        assert same_bits(got[near], true[near])
        assert (got[~near] >= true[~near]).all()  # never below the true distance (+inf >= +inf holds)
        print("query %d: cost %.3f, %d voxels, %d within the cost, %d rounds, %d tile visits"
              % (q, cost, full["path_len"][q], near.sum(), emu["stats"][q, 0], emu["stats"][q, 1]))


@pytest.mark.parametrize("case", gh.crafted_cases(), ids=lambda c: c["name"])
def test_return_codes(harness, case):
    """2.  every return code of the contract on crafted inputs, emulation and Dijkstra alike"""
    r = gh.run(harness, case["grid"], case["starts"], case["goals"], case["cap"], case["max_rounds"], sides=("full", "emu"))
    full, emu = r["full"], r["emu"]
    for q in range(len(case["starts"])):
        want = case["rtn"][q] if case["rtn"] is not None else full["rtn"][q]
        assert emu["rtn"][q] == want, (case["name"], q, emu["rtn"][q])
        if want == gh.ROUND_LIMIT:
            assert emu["path_len"][q] == 0 and np.isnan(emu["path_cost"][q])
            continue
        assert full["rtn"][q] == want
        assert emu["path_len"][q] == full["path_len"][q]
        assert same_bits(emu["path_cost"][q], full["path_cost"][q])
        assert np.array_equal(emu["paths"][q], full["paths"][q])
        if want == gh.BAD_ENDPOINT:
            assert emu["path_len"][q] == 0 and np.isnan(emu["path_cost"][q])
        if want == gh.NO_PATH:
            assert emu["path_len"][q] == 0 and np.isposinf(emu["path_cost"][q])
        if want == gh.OVERFLOW:
            assert emu["path_len"][q] > case["cap"] and len(emu["paths"][q]) == case["cap"]
            assert np.array_equal(emu["paths"][q][0], case["starts"][q])
        if want == gh.OK and (case["starts"][q] == case["goals"][q]).all():
            assert emu["path_len"][q] == 1 and emu["path_cost"][q] == 0.0


def test_tile_that_runs_out_of_sweeps_wakes_itself(tmp_path):
    """2.  The branch of a visit whose sweeps run out with changes left: the tile sets its OWN bit of the wake mask and goes on in
    the next round.  A build of the harness with 4 sweeps per visit reaches it on every crafted map, most plainly on the
    one-tile serpentine, where no neighbouring tile exists that could wake the tile instead.  Same fields, paths and codes."""
    few = gh.build(tmp_path, local_iters=4)
    for case in gh.crafted_cases():
        if case["max_rounds"]:
            continue
        r = gh.run(few, case["grid"], case["starts"], case["goals"], case["cap"], 0, sides=("full", "emu"))
        full, emu = r["full"], r["emu"]
        for q in range(len(case["starts"])):
            assert emu["rtn"][q] == full["rtn"][q] and emu["path_len"][q] == full["path_len"][q]
            assert np.array_equal(emu["paths"][q], full["paths"][q])
            if full["rtn"][q] == gh.BAD_ENDPOINT:
                continue
            assert same_bits(emu["path_cost"][q], full["path_cost"][q])
            near = full["dist"][q] <= (full["path_cost"][q] if full["rtn"][q] != gh.NO_PATH else np.inf)
            assert same_bits(emu["dist"][q][near], full["dist"][q][near]) and (emu["dist"][q][~near] >= full["dist"][q][~near]).all()
        if case["name"] == "tile_serpentine":
            assert case["grid"].shape == (8, 8, 8) and (full["path_len"] > 100).all()
            assert (emu["stats"][:, 0] >= 2).all() and (emu["stats"][:, 1] == emu["stats"][:, 0]).all()  # one tile, visited once per round


def check_path_properties(grid, start, goal, path, cost):
    """3.  26-neighbour steps, free voxels inside the map (the start excepted), the left fold of the weights equals the cost"""
    assert np.array_equal(path[0], start) and np.array_equal(path[-1], goal)
    step = np.abs(np.diff(path, axis=0))
    assert (step.max(axis=1) == 1).all()
    assert (path >= 0).all() and (path < np.array(grid.shape)).all()
    assert (grid[tuple(path[1:].T)] == 0).all()
    acc = 0.0
    for n in (step != 0).sum(axis=1):
        acc = acc + W[int(n)]
    assert same_bits(acc, cost)


def test_path_properties(harness, big):
    grid, starts, goals, r = big
    from tests.real_corridor_lib import LOWER, RES, grid_path
    for q in range(len(starts)):
        path, cost = r["emu"]["paths"][q], r["emu"]["path_cost"][q]
        check_path_properties(grid, starts[q], goals[q], path, cost)
        bfs = grid_path(grid, starts[q], goals[q])  # 4-connected, inside the z-slice: a walk of the graph, one unit per step
        assert bfs is not None and cost <= len(bfs) - 1
        assert np.array_equal(np.rint((bfs[0] - LOWER) / RES - 0.5).astype(int), starts[q])
    for case in gh.crafted_cases():
        o = gh.run(harness, case["grid"], case["starts"], case["goals"], 4096, 0, sides=("emu",), fields=False)["emu"]
        for q in range(len(case["starts"])):
            if o["rtn"][q] == gh.OK:
                check_path_properties(case["grid"], case["starts"][q], case["goals"][q], o["paths"][q], o["path_cost"][q])
