"""Clearance-aware grid paths (include/direct_cluster.h, "clearance-aware grid paths") on the CPU:
direct_amd/csrc/grid_path_clear_math.h compiled by g++ (tests/grid_path_clear_harness.py).  Every case runs on both sides of
that harness, the independent heap Dijkstra and the emulation of the tiled rounds, the latter also in a build with 4 sweeps per
visit so that tiles wake themselves.  1. neutral parameters against the existing harness, byte for byte; 2. the floor against the
existing harness on the thresholded map; 3. the penalty: emulation against Dijkstra, the fold, path_d2 / path_min_d2, and
conditions on the answer that keep the case from being vacuous; 4. a capped field."""
import numpy as np
import pytest

from tests import grid_path_clear_harness as ch
from tests import grid_path_harness as gh

W = {1: 1.0, 2: float(np.sqrt(2.0)), 3: float(np.sqrt(3.0))}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return gh.build(tmp_path_factory.mktemp("grid_path_plain"))


@pytest.fixture(scope="module")
def clear(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_path_clear")
    return ch.build(d), ch.build(d, local_iters=4)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bytes(new, old, q, dist):
    """one query of the new harness against one of the existing harness, every output they share"""
    assert new["rtn"][q] == old["rtn"][q] and new["path_len"][q] == old["path_len"][q], (q, new["rtn"][q], old["rtn"][q])
    assert bits(new["path_cost"][q]) == bits(old["path_cost"][q]) or (np.isnan(new["path_cost"][q]) and np.isnan(old["path_cost"][q]))
    assert np.array_equal(new["paths"][q], old["paths"][q])
    if dist:
        assert np.array_equal(bits(new["dist"][q]), bits(old["dist"][q]))


def check_outputs_at_the_path(r, d2, starts, q):
    """path_d2 / path_min_d2 are the field read at the path; the minimum leaves the start out"""
    p = r["paths"][q]
    assert np.array_equal(r["path_d2"][q], d2[tuple(p.T)] if len(p) else np.zeros(0, np.int32))
    if r["rtn"][q] == ch.OK and len(p) > 1:
        assert np.array_equal(p[0], starts[q]) and r["path_min_d2"][q] == d2[tuple(p[1:].T)].min()
    elif r["rtn"][q] != ch.OVERFLOW:
        assert r["path_min_d2"][q] == ch.DIST_NONE


def test_header_and_export_exist():
    import os
    from direct_amd import abi, cluster
    assert "direct_cluster_grid_path_clear_batch" in cluster.EXPORTS
    text = open(os.path.join(ch.ROOT, "include", "direct_cluster.h")).read()
    assert "direct_grid_path_clear_in_t" in text and "direct_grid_path_clear_out_t" in text
    assert os.path.exists(os.path.join(ch.ROOT, "direct_amd", "csrc", "grid_path_clear_math.h"))
    assert abi.GRID_PATH_MAX_PENALTY == 65536
    t = cluster.clearance_penalty_table(0.3, 4)
    assert len(t) == 16 and t[0] == 0.3 and np.array_equal(t, ch.soft_table(0.3, 4.0)) and (t > 0).all()
    assert len(cluster.clearance_penalty_table(1.0, 2.5)) == 7 and len(cluster.clearance_penalty_table(1.0, 0)) == 0


def neutral_cases():
    cases = [dict(c) for c in gh.crafted_cases()]
    g = gh.random_map((20, 17, 11), 21, 0.25)
    free = np.argwhere(g == 0)
    rng = np.random.default_rng(4)
    cases.append(dict(name="random_20x17x11", grid=g, cap=64, max_rounds=0, starts=free[rng.integers(len(free), size=8)].astype(np.int32),
                      goals=free[rng.integers(len(free), size=8)].astype(np.int32)))
    return cases


@pytest.mark.parametrize("case", neutral_cases(), ids=lambda c: c["name"])
def test_neutral_parameters_are_the_existing_harness(plain, clear, case):
    """1.  min_d2 = 0 and no table: the existing harness's result byte for byte, codes, paths, costs and both fields (the
    emulations visit the tiles in the same order, so even the pruned field agrees), on its crafted cases and a random
    20 x 17 x 11 map; adding 0.0 changes no bit"""
    grid = case["grid"]
    d2 = ch.brute_distance_field(grid)
    old = gh.run(plain, grid, case["starts"], case["goals"], case["cap"], case["max_rounds"], sides=("full", "emu"))
    for build in clear[:1] if case["max_rounds"] else clear:
        new = ch.run(build, grid, d2, case["starts"], case["goals"], 0, None, case["cap"], case["max_rounds"])
        for q in range(len(case["starts"])):
            same_bytes(new["full"], old["full"], q, dist=True)
            same_bytes(new["emu"], old["emu"], q, dist=build is clear[0])
            if new["emu"]["rtn"][q] not in (ch.ROUND_LIMIT, ch.BAD_ENDPOINT):
                same_bytes(new["emu"], new["full"], q, dist=False)
            for side in ("full", "emu"):
                check_outputs_at_the_path(new[side], d2, case["starts"], q)
        if build is clear[0]:
            assert np.array_equal(new["emu"]["stats"], old["emu"]["stats"])
    # a table of zeros and min_d2 = 1 are neutral too
    if not case["max_rounds"]:
        z = ch.run(clear[0], grid, d2, case["starts"], case["goals"], 1, np.zeros(5), case["cap"], 0)
        for q in range(len(case["starts"])):
            same_bytes(z["full"], old["full"], q, dist=True)
            same_bytes(z["emu"], old["emu"], q, dist=True)


@pytest.fixture(scope="module")
def walls():
    grid = ch.walls_map()
    d2 = ch.brute_distance_field(grid)
    s, g = ch.queries(grid, d2, 14, seed=1, floor=9)
    return grid, d2, s, g


@pytest.mark.parametrize("min_d2", [1, 2, 4, 9])
def test_floor_is_the_existing_harness_on_the_thresholded_map(plain, clear, walls, min_d2):
    """2.  walls with gaps of different widths: a floor equals the existing harness on byte | (D2 < min_d2), byte for byte; the
    query whose goal is below the floor has NO_PATH, the one whose START is below it still works"""
    grid, d2, s, g = walls
    # a voxel below this floor that touches one at or above it (D2 = k^2 at k voxels from the wall x = 6; for min_d2 = 1 only an
    # occupied voxel is below the floor): once as a goal, once as a START
    low = [{1: 6, 2: 5, 4: 5, 9: 4}[min_d2], 10, 5]
    assert d2[tuple(low)] < min_d2 <= d2[low[0] - 1, 10, 5]
    s = np.concatenate([s, [[2, 12, 6], low]]).astype(np.int32)
    g = np.concatenate([g, [low, [38, 12, 6]]]).astype(np.int32)
    thresholded = (grid | (d2 < min_d2)).astype(np.uint8)
    old = gh.run(plain, thresholded, s, g, 4096, 0, sides=("full", "emu"))
    for build in clear:
        new = ch.run(build, grid, d2, s, g, min_d2, None)
        for q in range(16):
            same_bytes(new["full"], old["full"], q, dist=True)
            same_bytes(new["emu"], old["emu"], q, dist=build is clear[0])
            same_bytes(new["emu"], new["full"], q, dist=False)
            for side in ("full", "emu"):
                check_outputs_at_the_path(new[side], d2, s, q)
                if new[side]["rtn"][q] == ch.OK and new[side]["path_len"][q] > 1:
                    assert new[side]["path_min_d2"][q] >= min_d2
    full = new["full"]
    assert (full["rtn"][:14] == ch.OK).all() and full["rtn"][15] == ch.OK
    assert full["rtn"][14] == ch.NO_PATH
    assert full["path_len"][14] == 0 and np.isposinf(full["path_cost"][14]) and full["path_min_d2"][14] == ch.DIST_NONE


def test_floors_move_the_paths(clear, walls):
    """2.  not vacuous: every floor of the list changes some path against the floor before it"""
    grid, d2, s, g = walls
    r = [ch.run(clear[0], grid, d2, s, g, m, None, sides=("full",), fields=False)["full"] for m in (0, 2, 4, 9, 10)]
    for a, b in zip(r[:-1], r[1:]):
        assert any(not np.array_equal(a["paths"][q], b["paths"][q]) for q in range(14))
        assert (b["path_cost"][:14] >= a["path_cost"][:14]).all()


def folds(path, d2, pen):
    """the cost of a path folded three ways: as defined ((c + w) + pen), with the pair grouped (c + (w + pen)), and with the
    penalty before the step weight ((c + pen) + w)"""
    c0 = c1 = c2 = 0.0
    for i in range(1, len(path)):
        w = W[int((path[i] != path[i - 1]).sum())]
        dd = d2[tuple(path[i])]
        p = float(pen[dd]) if dd < len(pen) else 0.0
        c0, c1, c2 = (c0 + w) + p, c1 + (w + p), (c2 + p) + w
    return c0, c1, c2


@pytest.fixture(scope="module")
def gap():
    grid = ch.gap_map()
    d2 = ch.brute_distance_field(grid)
    s, g = ch.queries(grid, d2, 16, seed=3)
    return grid, d2, s, g


@pytest.mark.parametrize("table", [(0.3, 4.0), (1.0, 4.0)], ids=["w0.3_r4", "w1.0_r4"])
def test_penalty(clear, gap, table):
    """3.  a direct gap one voxel wide and a detour through open space, a table of non-representable doubles"""
    grid, d2, s, g = gap
    pen = ch.soft_table(*table)
    assert len(pen) == 16 and not any(float(p).is_integer() for p in pen[1:])
    unpenalised = ch.run(clear[0], grid, d2, s, g, 0, None, sides=("full",), fields=False)["full"]
    differ = grouped = pen_first = 0
    for build in clear:
        r = ch.run(build, grid, d2, s, g, 0, pen)
        full, emu = r["full"], r["emu"]
        for q in range(16):
            assert full["rtn"][q] == ch.OK and emu["rtn"][q] == ch.OK
            assert bits(emu["path_cost"][q]) == bits(full["path_cost"][q])
            assert emu["path_len"][q] == full["path_len"][q] and np.array_equal(emu["paths"][q], full["paths"][q])
            near = full["dist"][q] <= full["path_cost"][q]
            assert np.array_equal(bits(emu["dist"][q][near]), bits(full["dist"][q][near]))
            assert (emu["dist"][q][~near] >= full["dist"][q][~near]).all()
            c0, c1, c2 = folds(emu["paths"][q], d2, pen)
            assert bits(c0) == bits(emu["path_cost"][q])
            for side in ("full", "emu"):
                check_outputs_at_the_path(r[side], d2, s, q)
                assert np.array_equal(r[side]["paths"][q][0], s[q]) and np.array_equal(r[side]["paths"][q][-1], g[q])
            if build is clear[0]:
                differ += not np.array_equal(emu["paths"][q], unpenalised["paths"][q])
                grouped += int(bits(c1)[0] != bits(c0)[0])
                pen_first += int(bits(c2)[0] != bits(c0)[0])
    print("table %s: %d of 16 paths differ from the unpenalised optimum, cost bits differ from d + (w + pen) for %d and from "
          "(d + pen) + w for %d; min D2 on the path %s (unpenalised %s)"
          % (table, differ, grouped, pen_first, emu["path_min_d2"].tolist(), unpenalised["path_min_d2"].tolist()))
    assert differ >= 8
    assert (emu["path_min_d2"] >= unpenalised["path_min_d2"]).all() and (emu["path_min_d2"] > unpenalised["path_min_d2"]).any()
    if table == (0.3, 4.0):  # on the harness's answer: the two additions and their order are visible in the bits
        assert grouped >= 1 and pen_first >= 1


def test_penalty_with_floor_and_small_capacity(clear, gap):
    """3.  floor and table together; a path_capacity that is too small reports the needed length and the whole path's minimum"""
    grid, d2, s, g = gap
    pen = ch.soft_table(0.3, 4.0)
    a = ch.run(clear[0], grid, d2, s, g, 2, pen)
    assert (a["full"]["rtn"] == ch.OK).all() and (a["full"]["path_min_d2"] >= 2).all()
    cap = int(a["full"]["path_len"].min()) - 1
    b = ch.run(clear[1], grid, d2, s, g, 2, pen, path_capacity=cap)
    for side in ("full", "emu"):
        assert (b[side]["rtn"] == ch.OVERFLOW).all()
        assert np.array_equal(b[side]["path_len"], a["full"]["path_len"]) and np.array_equal(b[side]["path_min_d2"], a["full"]["path_min_d2"])
        assert np.array_equal(bits(b[side]["path_cost"]), bits(a["full"]["path_cost"]))
        for q in range(16):
            assert np.array_equal(b[side]["paths"][q], a["full"]["paths"][q][:cap])
            assert np.array_equal(b[side]["path_d2"][q], a["full"]["path_d2"][q][:cap])


@pytest.mark.parametrize("cap_vox,min_d2,n_pen", [(4, 9, 16), (4, 16, 0), (3, 0, 9), (5, 4, 16)])
def test_capped_field(clear, gap, cap_vox, min_d2, n_pen):
    """4.  a field stored as min(D2, cap2) gives the uncapped field's results whenever min_d2 <= cap2 and n_penalty <= cap2
    (path_d2 / path_min_d2 report the STORED values, so they are the uncapped ones capped)"""
    grid, d2, s, g = gap
    capped = ch.brute_distance_field(grid, cap_vox)
    cap2 = cap_vox * cap_vox
    assert capped.max() == cap2 and min_d2 <= cap2 and n_pen <= cap2 and np.array_equal(capped, np.minimum(d2, cap2))
    pen = ch.soft_table(0.3, 4.0)[:n_pen]
    a = ch.run(clear[0], grid, d2, s, g, min_d2, pen)
    b = ch.run(clear[0], grid, capped, s, g, min_d2, pen)
    for side in ("full", "emu"):
        for k in ("rtn", "path_len", "stats"):
            assert np.array_equal(a[side][k], b[side][k]), k
        assert np.array_equal(bits(a[side]["path_cost"]), bits(b[side]["path_cost"]))
        assert np.array_equal(bits(a[side]["dist"]), bits(b[side]["dist"]))
        none = a[side]["path_min_d2"] == ch.DIST_NONE
        assert np.array_equal(np.where(none, ch.DIST_NONE, np.minimum(a[side]["path_min_d2"], cap2)), b[side]["path_min_d2"])
        for q in range(16):
            assert np.array_equal(a[side]["paths"][q], b[side]["paths"][q])
            assert np.array_equal(np.minimum(a[side]["path_d2"][q], cap2), b[side]["path_d2"][q])
    assert (a["full"]["rtn"] == ch.OK).sum() >= 8
