"""Shared-start grid paths (include/direct_cluster.h, "shared-start grid paths") on the CPU: direct_amd/csrc/grid_path_fan_math.h
compiled by g++ (tests/grid_path_fan_harness.py), the fan's rounds by lane-loop emulation.  Four builds - the library's sweeps per
visit and 4 (tiles wake themselves), the bound refreshed before every round and before every eighth - must give the same bytes per
goal, and every goal is held against the independent heap Dijkstra of the existing harnesses run on the PAIR (source, goal): the
plain one in neutral mode, the clear one otherwise.  `dist` is held against that Dijkstra's field under the contract's rule."""
import os

import numpy as np
import pytest

from tests import grid_path_clear_harness as ch
from tests import grid_path_fan_harness as fh
from tests import grid_path_harness as gh


@pytest.fixture(scope="module")
def fan(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_path_fan")
    return [fh.build(d, li, be) for li in (None, 4) for be in (1, 8)]


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return gh.build(tmp_path_factory.mktemp("fan_ref_plain")), ch.build(tmp_path_factory.mktemp("fan_ref_clear"))


def run_all(fan, grid, sources, goals, goal_src, d2=None, min_d2=0, penalty=None, cap=4096, max_rounds=0):
    """the four builds; asserts that they agree on every per-goal byte and returns the first build's result"""
    clear = fh.is_clear(min_d2, penalty)
    res = [fh.run(b, grid, sources, goals, goal_src, d2, min_d2, penalty, cap, max_rounds) for b in fan]
    for r in res[1:]:
        fh.same_per_goal(r, res[0], clear, "builds")
    return res[0]


def check(fan, refs, grid, sources, goals, goal_src, d2=None, min_d2=0, penalty=None, cap=4096, where=""):
    """fan == pairwise Dijkstra for every goal, and the dist contract; -> (fan result, pairwise result, worst eligible cost per source)"""
    clear = fh.is_clear(min_d2, penalty)
    if clear and d2 is None:
        d2 = ch.brute_distance_field(grid)
    got = run_all(fan, grid, sources, goals, goal_src, d2, min_d2, penalty, cap)
    ref = fh.pairwise(refs[0], refs[1], grid, sources, goals, goal_src, d2, min_d2, penalty, cap)
    fh.same_per_goal(got, ref, clear, where)
    worst = fh.check_dist(got, ref, grid, sources, goals, goal_src, d2, min_d2, clear, where)
    return got, ref, worst


def test_header_export_and_binding_exist():
    from direct_amd import abi, cluster
    assert "direct_cluster_grid_path_fan_batch" in cluster.EXPORTS and hasattr(cluster.ClusterGenerator, "grid_paths_fan")
    text = open(os.path.join(fh.ROOT, "include", "direct_cluster.h")).read()
    assert "direct_grid_path_fan_in_t" in text and "direct_grid_path_fan_out_t" in text
    for name in ("grid_path_fan.h", "grid_path_fan_math.h"):
        assert os.path.exists(os.path.join(fh.ROOT, "direct_amd", "csrc", name))
    assert [n for n, _ in abi.GridPathFanOut._fields_] == list(abi.GRID_PATH_FAN_OUTPUTS)


@pytest.mark.parametrize("case", gh.crafted_cases(), ids=lambda c: c["name"])
def test_crafted_cases_regrouped_by_start(fan, refs, case):
    """the existing harness's crafted cases, the pairs regrouped by start: every return code, partial tiles, a flat map, the maze, an
    occupied start, start == goal, a capacity that is too small, the round cap"""
    sources, goals, gs = fh.regroup_by_start(case["starts"], case["goals"])
    if case["max_rounds"]:
        got = run_all(fan[:1], case["grid"], sources, goals, gs, cap=case["cap"], max_rounds=case["max_rounds"])
        assert list(got["rtn"]) == case["rtn"]      # ROUND_LIMIT for both goals of the far source, OK for the source that is its own goal
        assert got["path_len"][1] == 1 and got["path_cost"][1] == 0.0
        return
    got, _, _ = check(fan, refs, case["grid"], sources, goals, gs, cap=case["cap"], where=case["name"])
    if case["rtn"] is not None:
        assert list(got["rtn"]) == case["rtn"]


def random_fan(grid, n_src, per, seed):
    """n_src free sources and per goals each, drawn over ALL voxels of the map (occupied ones included: they are NO_PATH)"""
    rng = np.random.default_rng(seed)
    free = np.argwhere(grid == 0)
    every = np.argwhere(np.ones(grid.shape, bool))
    sources = free[rng.choice(len(free), n_src, replace=False)].astype(np.int32)
    goals = every[rng.integers(len(every), size=n_src * per)].astype(np.int32)
    return sources, goals, np.repeat(np.arange(n_src, dtype=np.int32), per)


@pytest.mark.parametrize("mode", ["neutral", "floor", "table"])
def test_random_map_three_sources_forty_goals(fan, refs, mode):
    """20 x 17 x 11, no dimension a multiple of the tile; 3 sources x 40 goals"""
    grid = gh.random_map((20, 17, 11), 21, 0.25)
    sources, goals, gs = random_fan(grid, 3, 40, seed=8)
    kw = dict(neutral={}, floor=dict(min_d2=2), table=dict(min_d2=1, penalty=ch.soft_table(0.3, 2.0)))[mode]
    got, _, _ = check(fan, refs, grid, sources, goals, gs, cap=64, where=mode, **kw)
    assert (got["rtn"] == fh.NO_PATH).sum() > 10 and (mode == "floor" or (got["rtn"] == fh.OK).sum() > 30)


def test_sealed_box_source_outside_goals_on_both_sides(fan, refs):
    """an eligible goal that is unreachable (a free voxel of the sealed room) switches pruning off: the whole component of the source
    is exact, the room's goals are NO_PATH, the others stay exact"""
    grid = gh.sealed_box_map()
    sources = np.array([[0, 0, 0]], np.int32)
    goals = np.array([[7, 8, 5], [19, 17, 11], [5, 6, 3], [2, 2, 2], [9, 10, 7], [4, 5, 2]], np.int32)   # room, far, room, near, room, shell
    got, ref, worst = check(fan, refs, grid, sources, goals, None, cap=64)
    assert list(got["rtn"]) == [fh.NO_PATH, fh.OK, fh.NO_PATH, fh.OK, fh.NO_PATH, fh.NO_PATH]
    assert np.isinf(worst[0])
    assert np.array_equal(got["dist"][0].view(np.int64), ref["dist"][0].view(np.int64))   # pruning off: the whole field is Dijkstra's


def side_fans(grid, d2, floor):
    """two sources, one on each side of the map along x, and 28 goals on both sides, every one with D2 >= floor"""
    s, g = ch.queries(grid, d2, 14, seed=1, floor=floor)
    left = s[s[:, 0] < 5][0] if (s[:, 0] < 5).any() else g[g[:, 0] < 5][0]
    right = s[s[:, 0] >= 35][0] if (s[:, 0] >= 35).any() else g[g[:, 0] >= 35][0]
    goals = np.concatenate([g, s])
    return np.array([left, right], np.int32), goals.astype(np.int32), (np.arange(len(goals)) % 2).astype(np.int32)


@pytest.mark.parametrize("min_d2", [1, 2, 4, 9])
def test_walls_with_floors(fan, refs, min_d2):
    """the floor closes the narrow gaps one after the other; min_d2 = 1 is neutral mode and is held against the PLAIN Dijkstra"""
    grid = ch.walls_map()
    d2 = ch.brute_distance_field(grid)
    sources, goals, gs = side_fans(grid, d2, 9)
    got, _, _ = check(fan, refs, grid, sources, goals, gs, d2=d2, min_d2=min_d2, cap=256, where="floor %d" % min_d2)
    assert (got["rtn"] == fh.OK).all()
    if min_d2 > 1:
        assert (got["path_min_d2"][got["path_len"] > 1] >= min_d2).all()


def test_gap_map_with_the_soft_table(fan, refs):
    grid = ch.gap_map()
    d2 = ch.brute_distance_field(grid)
    sources, goals, gs = side_fans(grid, d2, 0)
    got, _, _ = check(fan, refs, grid, sources, goals, gs, d2=d2, penalty=ch.soft_table(), cap=256)
    assert (got["rtn"] == fh.OK).all()
    plain, _, _ = check(fan, refs, grid, sources, goals, gs, cap=256)
    moved = [j for j in range(len(goals)) if not np.array_equal(got["paths"][j], plain["paths"][j])]
    assert len(moved) > len(goals) // 4 and (got["path_cost"][moved] > plain["path_cost"][moved]).all()   # the penalty moves paths


# ---- the named cases, in both modes --------------------------------------------------------------------------------------

MODES = {"neutral": {}, "clear": dict(min_d2=2, penalty=ch.soft_table(0.3, 3.0))}


@pytest.fixture(scope="module")
def named_map():
    grid = ch.walls_map()
    return grid, ch.brute_distance_field(grid)


@pytest.mark.parametrize("mode", list(MODES))
def test_goal_equal_to_an_occupied_source(fan, refs, named_map, mode):
    grid, d2 = named_map
    assert grid[6, 0, 5] == 1
    sources = np.array([[6, 0, 5]], np.int32)
    goals = np.array([[6, 0, 5], [3, 8, 5]], np.int32)
    got, _, _ = check(fan, refs, grid, sources, goals, None, d2=d2, cap=64, **MODES[mode])
    assert got["rtn"][0] == fh.OK and got["path_len"][0] == 1 and got["path_cost"][0] == 0.0
    assert got["rtn"][1] == (fh.OK if mode == "neutral" else fh.NO_PATH)   # the wall's free neighbours lie below the floor


@pytest.mark.parametrize("mode", list(MODES))
def test_an_occupied_goal_leaves_pruning_on(fan, refs, named_map, mode):
    """a goal that is NO_PATH before anything runs is not eligible: the bound is the worst of the OTHER goals, and the field beyond it
    is never relaxed - some voxel farther than the worst eligible goal is still +inf"""
    grid, d2 = named_map
    sources = np.array([[2, 10, 5]], np.int32)
    goals = np.array([[4, 12, 6], [6, 1, 5], [1, 6, 3], [0, 0, 0]], np.int32)   # [6, 1, 5] is wall, [0, 0, 0] is clutter
    assert grid[6, 1, 5] == 1 and grid[0, 0, 0] == 1
    got, ref, worst = check(fan, refs, grid, sources, goals, None, d2=d2, cap=64, **MODES[mode])
    assert list(got["rtn"]) == [fh.OK, fh.NO_PATH, fh.OK, fh.NO_PATH]
    true = ref["dist"][0]
    assert worst[0] == max(got["path_cost"][0], got["path_cost"][2])
    # The builds that refresh the bound before every round (the library's setting).  Refreshed once per eight rounds the bound is the
    # initial +inf for the first eight, which cover this map of 5 x 3 x 2 tiles: there the contract alone holds (check above).
    for b in (fan[0], fan[2]):
        dist = fh.run(b, grid, sources, goals, None, d2, path_capacity=64, **MODES[mode])["dist"][0]
        pruned = np.isinf(dist) & np.isfinite(true)
        assert pruned.sum() > grid.size // 4 and (true[pruned] > worst[0]).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_bad_endpoints_empty_source_duplicates_and_twin_sources(fan, refs, named_map, mode):
    """one call: a goal outside the map (that goal only), a source outside the map (all its goals, the other sources unaffected), a
    source with no goal, duplicate goals (identical bytes), two sources on one voxel (identical bytes)"""
    grid, d2 = named_map
    sources = np.array([[2, 10, 5], [40, 0, 0], [30, 3, 3], [2, 10, 5], [-1, 5, 5]], np.int32)   # source 2 has no goal
    goals = np.array([[10, 12, 6], [3, 24, 0], [10, 12, 6], [1, 1, 1], [2, 2, 2], [10, 12, 6], [38, 20, 9], [2, 10, 5]], np.int32)
    gs = np.array([0, 0, 0, 1, 1, 3, 3, 4], np.int32)
    got, _, worst = check(fan, refs, grid, sources, goals, gs, d2=d2, cap=128, **MODES[mode])
    assert list(got["rtn"]) == [fh.OK, fh.BAD_ENDPOINT, fh.OK, fh.BAD_ENDPOINT, fh.BAD_ENDPOINT, fh.OK, fh.OK, fh.BAD_ENDPOINT]
    assert np.array_equal(got["paths"][0], got["paths"][2]) and np.array_equal(got["paths"][0], got["paths"][5])
    assert got["path_cost"][0] == got["path_cost"][2] == got["path_cost"][5]
    assert worst[1] is None and worst[2] is None and worst[4] is None
    assert got["stats"][1].tolist() == [0, 0] and got["stats"][4].tolist() == [0, 0]        # a source outside the map computes nothing
    assert got["bound"][2] == 0.0 and got["stats"][2].tolist() == [1, 1]                    # no goal: bound 0, the start tile's one visit
    d = got["dist"][2]
    assert np.isinf(d).sum() == grid.size - 1 and d[np.ravel_multi_index((30, 3, 3), grid.shape)] == 0.0   # ... which relaxes nothing


@pytest.mark.parametrize("mode", list(MODES))
def test_capacity_one_too_small(fan, refs, named_map, mode):
    grid, d2 = named_map
    sources = np.array([[2, 10, 5]], np.int32)
    goals = np.array([[25, 5, 5], [4, 10, 5]], np.int32)
    full, _, _ = check(fan, refs, grid, sources, goals, None, d2=d2, cap=256, **MODES[mode])
    need = int(full["path_len"][0])
    got, _, _ = check(fan, refs, grid, sources, goals, None, d2=d2, cap=need - 1, **MODES[mode])
    assert list(got["rtn"]) == [fh.OVERFLOW, fh.OK] and got["path_len"][0] == need and got["path_cost"][0] == full["path_cost"][0]
    assert np.array_equal(got["paths"][0], full["paths"][0][:need - 1])
    if mode == "clear":
        assert got["path_min_d2"][0] == full["path_min_d2"][0] == d2[tuple(full["paths"][0][1:].T)].min()   # the WHOLE path's minimum


@pytest.mark.parametrize("mode", list(MODES))
def test_round_limit_names_exactly_the_sources_still_active(fan, named_map, mode):
    grid, d2 = named_map
    sources = np.array([[2, 10, 5], [30, 3, 3], [38, 20, 9]], np.int32)
    goals = np.array([[38, 20, 9], [2, 10, 5], [30, 3, 3], [3, 10, 5], [38, 20, 9]], np.int32)
    gs = np.array([0, 0, 1, 0, 2], np.int32)
    got = run_all(fan, grid, sources, goals, gs, d2=d2, cap=256, max_rounds=1, **MODES[mode])
    assert list(got["rtn"]) == [fh.ROUND_LIMIT, fh.ROUND_LIMIT, fh.OK, fh.ROUND_LIMIT, fh.OK]   # EVERY goal of source 0, its own voxel included
    assert (got["path_len"][[0, 1, 3]] == 0).all() and np.isnan(got["path_cost"][[0, 1, 3]]).all()
    assert got["path_len"][2] == 1 and got["path_len"][4] == 1
