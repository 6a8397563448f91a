"""The fan mode of the one program of tests/grid_path_harness.py (direct_amd/csrc/grid_path_fan_math.h compiled by g++) - TEST
INFRASTRUCTURE of tests/test_grid_path_fan_restatement.py and tests/test_gpu_grid_path_fan.py.  The C++ lives there: its fan driver
(one field per source, the bound of a source as k_fan_bound makes it, refreshed before every round or before every batch of eight -
a build option, as the sweeps per visit -, the host's batches of eight rounds) over the SAME visit and walk as the pair sides, with
fan == true (lim = bound[s]) and clear as is_clear() says.  This module is build / run wrappers and the checks the tests share.
The independent side is not the fan's: the tests hold every goal against the heap Dijkstra ("full") of that program run on the
pair, through tests/grid_path_harness.py in neutral mode and tests/grid_path_clear_harness.py in clear mode."""
import os

import numpy as np

from tests import grid_path_harness as gh

ROOT = gh.ROOT
OK, NO_PATH, BAD_ENDPOINT, OVERFLOW, ROUND_LIMIT = gh.OK, gh.NO_PATH, gh.BAD_ENDPOINT, gh.OVERFLOW, gh.ROUND_LIMIT
DIST_NONE = 0x7fffffff


def build(workdir, local_iters=None, bound_every=1):
    """local_iters: sweeps per tile visit (DIRECT_GRIDPATH_LOCAL_ITERS; None: the library's); bound_every: 1 or 8, rounds between
    two refreshes of the bound"""
    return gh.build_program(workdir, local_iters, bound_every)


def is_clear(min_d2, penalty):
    return not (int(min_d2) <= 1 and (penalty is None or len(penalty) == 0))


def run(harness, grid, sources, goals, goal_src=None, d2=None, min_d2=0, penalty=None, path_capacity=4096, max_rounds=0, fields=True):
    """-> dict(rtn, path_len, path_cost, path_min_d2, paths: list of [n][3], path_d2: list of [n] (per goal); stats [S][2], bound [S],
    dist [S][G] or None (per source)).  Neutral mode (min_d2 <= 1, no table) needs no d2."""
    sources = np.ascontiguousarray(sources, np.int32).reshape(-1, 3)
    goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
    S, n, G = len(sources), len(goals), np.asarray(grid).size
    fout = gh.execute(harness, True, grid, sources, goals, np.zeros(n, np.int32) if goal_src is None else goal_src, path_capacity,
                      max_rounds, (), fields, clear=is_clear(min_d2, penalty), d2=d2, min_d2=min_d2, penalty=penalty)
    per_goal = gh.new_paths(n)
    r = dict({k: per_goal[k] for k in ("rtn", "path_len", "path_cost", "path_min_d2", "paths", "path_d2")},
             stats=np.zeros((S, 2), np.int32), bound=np.zeros(S), dist=np.zeros((S, G)) if fields else None)
    with open(fout, "rb") as f:
        for j in range(n):
            gh.read_path(f, path_capacity, per_goal, j)
        for s in range(S):
            r["stats"][s] = np.fromfile(f, np.int32, 2)
            r["bound"][s] = np.fromfile(f, np.float64, 1)[0]
            if fields:
                r["dist"][s] = np.fromfile(f, np.float64, G)
        assert f.read() == b""
    os.remove(fout)
    return r


def pairwise(ref_plain, ref_clear, grid, sources, goals, goal_src=None, d2=None, min_d2=0, penalty=None, path_capacity=4096):
    """every (sources[goal_src[j]], goals[j]) pair through the independent heap Dijkstra ("full") of the existing harnesses: the plain
    one in neutral mode, the clear one otherwise.  -> its dict, per goal, with dist [n][G] (the WHOLE component, exact)"""
    from tests import grid_path_clear_harness as gch
    sources = np.asarray(sources, np.int32).reshape(-1, 3)
    goals = np.asarray(goals, np.int32).reshape(-1, 3)
    gs = np.zeros(len(goals), np.int32) if goal_src is None else np.asarray(goal_src, np.int32)
    starts = sources[gs]
    if is_clear(min_d2, penalty):
        return gch.run(ref_clear, grid, d2, starts, goals, min_d2=min_d2, penalty=penalty, path_capacity=path_capacity, sides=("full",))["full"]
    return gh.run(ref_plain, grid, starts, goals, path_capacity=path_capacity, sides=("full",))["full"]


def same_per_goal(got, ref, clear, where=""):
    """the per-goal outputs of a fan result (host layout) against a pairwise result: codes, lengths, costs and paths to the bit"""
    n = len(ref["rtn"])
    assert np.array_equal(got["rtn"], ref["rtn"]), (where, got["rtn"], ref["rtn"])
    assert np.array_equal(got["path_len"], ref["path_len"]), where
    a, b = np.ascontiguousarray(got["path_cost"], np.float64), np.ascontiguousarray(ref["path_cost"], np.float64)
    assert ((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all(), (where, a, b)
    for j in range(n):
        assert np.array_equal(got["paths"][j], ref["paths"][j]), (where, j)
    if clear:
        assert np.array_equal(got["path_min_d2"], ref["path_min_d2"]), where
        for j in range(n):
            assert np.array_equal(got["path_d2"][j], ref["path_d2"][j]), (where, j)


def check_dist(got, ref, grid, sources, goals, goal_src, d2=None, min_d2=0, clear=False, where=""):
    """the dist contract per source: exact against the Dijkstra field wherever the true distance is <= the largest path_cost among the
    source's eligible goals (all of the component if one of them is unreachable), >= the true distance elsewhere.  ref: pairwise()'s
    result (its field of any goal of the source is the source's whole component).  -> per source the worst eligible cost (None
    without a goal inside the map)"""
    sources = np.asarray(sources).reshape(-1, 3)
    goals = np.asarray(goals).reshape(-1, 3)
    gs = np.zeros(len(goals), np.int32) if goal_src is None else np.asarray(goal_src)
    dims = np.array(grid.shape)
    worst = []
    for s in range(len(sources)):
        src = sources[s]
        if ((src < 0) | (src >= dims)).any():
            worst.append(None)
            continue
        mine = [j for j in range(len(goals)) if gs[j] == s and not ((goals[j] < 0) | (goals[j] >= dims)).any()]
        if not mine:
            worst.append(None)
            continue
        true = ref["dist"][mine[0]]
        lim = 0.0
        for j in mine:
            g = tuple(goals[j])
            ok = (goals[j] == src).all() or (grid[g] == 0 and (not clear or d2[g] >= min_d2))
            if ok:
                lim = max(lim, true[np.ravel_multi_index(g, grid.shape)])
        worst.append(lim)
        mine_d = got["dist"][s]
        sel = true <= lim
        assert np.array_equal(mine_d[sel].view(np.int64), true[sel].view(np.int64)), (where, s)
        assert (mine_d >= true).all(), (where, s)
    return worst


def regroup_by_start(starts, goals):
    """(start, goal) pairs -> sources (the distinct starts, in order of first appearance), goals, goal_src"""
    starts = np.asarray(starts, np.int32).reshape(-1, 3)
    keys, sources, gs = {}, [], []
    for s in starts:
        k = tuple(int(v) for v in s)
        if k not in keys:
            keys[k] = len(sources)
            sources.append(k)
        gs.append(keys[k])
    return np.array(sources, np.int32), np.asarray(goals, np.int32).reshape(-1, 3), np.array(gs, np.int32)
