"""One sensor scan folded into the map (include/direct_cluster.h, "one sensor scan folded into the map") on the CPU:
direct_amd/csrc/map_scan_math.h compiled by g++ as a program that emulates the kernels as lane loops (tests/map_scan_harness.py),
plain and under the address and undefined-behaviour sanitizers, against a restatement in pure Python floats written from the
definition's text - byte for byte (grids are bytes and stats are counts: there are no tolerances); an independent geometric check of
the restatement's rays; and the scenario the call exists for: a wall that a later scan looks through leaves the map."""
import math
import os

import numpy as np
import pytest

from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh

ROOT = sh.ROOT
INFLATES = ((0, 0, 0), (2, 2, 1))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("map_scan"))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("map_scan_san"), sanitize=True)


@pytest.fixture(scope="module")
def clouds():
    return sh.clouds()


@pytest.fixture(scope="module")
def wanted(clouds):
    """the restatement of every (cloud, range) once, on an empty scan grid, shared by the tests below and left unchanged"""
    return {(name, r): sh.restate(pts, sh.ORIGIN, r) for name, pts in clouds.items() for r in sh.RANGES}


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "raw", int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1]), (what, "map", int((got[1] != want[1]).sum()))
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])


@pytest.mark.parametrize("max_range", sh.RANGES)
def test_header_program_equals_the_restatement(harness, clouds, wanted, max_range):
    """on a FULL scan grid too (every byte 1), where the carve is what shows, and with both strides"""
    full = np.ones(sh.DIMS, np.uint8)
    for name, pts in clouds.items():
        same(sh.run(harness, pts, sh.ORIGIN, max_range), wanted[name, max_range], (name, "empty"))
        want = sh.restate(pts, sh.ORIGIN, max_range, (2, 2, 1), raw=full, before=full)
        assert (want[0] == 0).any() and (name != "random" or max_range < 1.0 or want[2][7] > 0)   # carved; a hole of 1.5 m outlives the dilation
        for stride in (3, 4):
            got = sh.run(harness, pts if stride == 3 else mh.with_stride4(pts), sh.ORIGIN, max_range, (2, 2, 1), raw=full, before=full)
            same(got, want, (name, "full", stride))


def test_header_program_under_the_sanitizers(sanitized, clouds, wanted):
    """the same program built with -fsanitize=address,undefined (no recovery: a finding is a non-zero exit), stand-alone"""
    every = np.concatenate(list(clouds.values()))
    for r in sh.RANGES:
        for name, pts in clouds.items():
            same(sh.run(sanitized, pts, sh.ORIGIN, r), wanted[name, r], (name, r))
        for inflate in ((2, 2, 1), (64, 64, 64)):
            same(sh.run(sanitized, every, sh.ORIGIN, r, inflate), sh.restate(every, sh.ORIGIN, r, inflate), (r, inflate))
    # an origin on voxel faces, and one in the last voxel of every axis
    for origin in (sh.LOWER + np.array([20, 18, 6]) * sh.RES, sh.LOWER + (np.array(sh.DIMS) - 0.5) * sh.RES):
        same(sh.run(sanitized, every, origin, 1.5), sh.restate(every, origin, 1.5), origin)


def test_an_origin_on_voxel_faces_and_in_a_corner(harness, clouds):
    every = np.concatenate(list(clouds.values()))
    full = np.ones(sh.DIMS, np.uint8)
    for origin in (sh.LOWER + np.array([20, 18, 6]) * sh.RES, sh.LOWER + (np.array(sh.DIMS) - 0.5) * sh.RES, sh.LOWER.copy()):
        for r in sh.RANGES:
            same(sh.run(harness, every, origin, r, raw=full), sh.restate(every, origin, r, raw=full), (origin, r))


def meets(cell, o, d, t_end, eps=1e-9):
    """the closed cube of a voxel, widened by eps, against the segment o + t d, 0 <= t <= t_end: the slab test"""
    t0, t1 = 0.0, t_end
    for a in range(3):
        lo = float(sh.LOWER[a]) + cell[a] * sh.RES - eps
        hi = float(sh.LOWER[a]) + (cell[a] + 1) * sh.RES + eps
        if d[a] == 0.0:
            if not (lo <= o[a] <= hi):
                return False
            continue
        ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return t0 <= t1


def test_geometry_of_the_restated_rays(clouds):
    """independent of the walk's own arithmetic: the first voxel is the origin's, consecutive voxels are face neighbours and none
    repeats, a hit inside the map ends in its point's voxel, and every cleared voxel's closed cube meets the segment (to the
    range's end for a truncated ray), widened by 1e-9 m for the rounding of tmax"""
    o = [float(v) for v in sh.ORIGIN]
    start = tuple(sh.origin_voxel(sh.ORIGIN, sh.DIMS, sh.RES, sh.LOWER, sh.UPPER))
    assert start == (22, 16, 6)
    kinds = {sh.HIT: 0, sh.TRUNCATED: 0, sh.SKIPPED: 0}
    inside_hits = left_early = 0
    for r in sh.RANGES:
        for name, pts in clouds.items():
            for p in pts:
                kind, cleared, end = sh.walk(p, sh.ORIGIN, r)
                kinds[kind] += 1
                if kind == sh.SKIPPED:
                    assert not cleared and not np.isfinite(p).all()
                    continue
                e = [float(v) for v in p]
                d = [e[a] - o[a] for a in range(3)]
                length = math.sqrt(sum(v * v for v in d))
                assert (kind == sh.HIT) == (length <= r) or abs(length - r) < 1e-12
                chain = cleared + ([end] if kind == sh.HIT else [])
                assert chain[0] == start, (name, p)
                assert len(set(cleared)) == len(cleared)
                for u, v in zip(chain, chain[1:]):
                    assert sum(abs(u[a] - v[a]) for a in range(3)) == 1, (name, p, u, v)
                assert all(0 <= c[a] < sh.DIMS[a] for c in cleared for a in range(3))
                t_end = 1.0 if kind == sh.HIT else r / length
                for c in cleared:
                    assert meets(c, o, d, t_end), (name, p, r, c)
                if kind == sh.HIT:
                    inside = all(sh.LOWER[a] <= e[a] < sh.LOWER[a] + sh.DIMS[a] * sh.RES for a in range(3))
                    if inside and all(0 <= end[a] < sh.DIMS[a] for a in range(3)):
                        inside_hits += 1
                        assert meets(end, e, [0.0, 0.0, 0.0], 0.0), (name, p, end)   # the point lies in the closed cube of `end`
                        assert end == tuple(int(math.floor((e[a] - float(sh.LOWER[a])) * (1.0 / sh.RES))) for a in range(3))
                    elif inside:
                        raise AssertionError(("a hit inside the map ended outside it", name, p, end))
                else:
                    tip = [o[a] + t_end * d[a] for a in range(3)]   # where the range ends
                    left_early += not all(sh.LOWER[a] <= tip[a] < sh.LOWER[a] + sh.DIMS[a] * sh.RES for a in range(3))
    assert kinds[sh.HIT] > 2500 and kinds[sh.TRUNCATED] > 2500 and kinds[sh.SKIPPED] == 15 and inside_hits > 1500
    assert left_early > 20  # truncated rays that left the map before their range ended


def test_order_and_phases(harness, clouds):
    """all carving precedes all marking: a return survives the rays of the same scan that pass through its voxel, in any order"""
    near = (sh.LOWER + (np.array([25, 16, 6]) + 0.5) * sh.RES).astype(np.float32)
    far = (sh.LOWER + (np.array([31, 16, 6]) + 0.5) * sh.RES).astype(np.float32)   # its ray passes through voxel (25, 16, 6)
    for pts in (np.stack([near, far]), np.stack([far, near])):
        for raw, _, stats in (sh.restate(pts, sh.ORIGIN, 10.0), sh.run(harness, pts, sh.ORIGIN, 10.0)[:3]):
            assert raw[25, 16, 6] == 1 and raw[31, 16, 6] == 1 and stats[4] == 2
    pts = clouds["random"]
    want = sh.restate(pts, sh.ORIGIN, 1.5, (2, 2, 1))
    same(sh.run(harness, pts[np.random.default_rng(3).permutation(len(pts))], sh.ORIGIN, 1.5, (2, 2, 1))[:3], want, "shuffled")


def test_inflation_is_a_voxel_box_without_wrap(harness):
    corner = (sh.LOWER + (np.array([[0, 0, 0], [39, 35, 11], [22, 0, 11]]) + 0.5) * sh.RES).astype(np.float32)
    for inflate in ((0, 0, 0), (2, 2, 1), (1, 0, 3), (64, 64, 64)):
        raw, new, stats = sh.restate(corner, sh.ORIGIN, 10.0, inflate)
        same(sh.run(harness, corner, sh.ORIGIN, 10.0, inflate)[:3], (raw, new, stats), inflate)
        want = np.zeros(sh.DIMS, np.uint8)
        for v in np.argwhere(raw == 1):
            lo, hi = np.maximum(v - inflate, 0), v + inflate + 1
            want[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
        assert np.array_equal(new, want) and stats[4] == 3 and stats[5] == want.sum() == stats[6] and stats[7] == 0
    assert sh.restate(corner, sh.ORIGIN, 10.0, (64, 64, 64))[1].all()


@pytest.mark.parametrize("inflate", INFLATES)
def test_a_wall_that_a_later_scan_looks_through_is_gone(harness, inflate):
    """scan 1 sees a wall; scan 2, from the same origin, sees the room behind it: the wall's voxels are gone, and with them their
    shell.  A wall only ADDed by map_from_cloud and then adopted behaves the same."""
    wpts, room, wall = sh.wall_and_room()
    w = tuple(wall.T)
    raw1, map1, s1 = sh.restate(wpts, sh.ORIGIN, 10.0, inflate)
    assert raw1[w].all() and s1[4] == len(wall) and s1[6] == map1.sum() and s1[7] == 0
    shell = sh.dilate(raw1, inflate) == 1
    assert np.array_equal(map1 == 1, shell) and (inflate == (0, 0, 0) or shell.sum() > 3 * len(wall))
    raw2, map2, s2 = sh.restate(room, sh.ORIGIN, 10.0, inflate, raw=raw1, before=map1)
    assert not raw2[w].any() and not raw2[:36].any() and raw2[36].any()
    assert not map2[shell].any() and s2[7] == shell.sum()           # the shell left with the wall
    same(sh.run(harness, room, sh.ORIGIN, 10.0, inflate, raw=raw1, before=map1)[:3], (raw2, map2, s2), "continue")
    # the same scan again changes nothing: stats[6] + stats[7] == 0 is what keeps the field
    raw3, map3, s3 = sh.restate(room, sh.ORIGIN, 10.0, inflate, raw=raw2, before=map2)
    assert np.array_equal(map3, map2) and s3[6] == 0 and s3[7] == 0
    # ADD by map_from_cloud (margin 0: one voxel up and down in z), then ADOPT
    added, _ = mh.restate(wpts, 0.0, mh.CLAMP)
    assert added[w].all() and added.sum() > len(wall)
    raw4, map4, s4 = sh.restate(room, sh.ORIGIN, 10.0, inflate, raw=added, before=added)
    assert not raw4[:36].any() and not map4[added == 1].any() and s4[7] == added.sum()
    same(sh.run(harness, room, sh.ORIGIN, 10.0, inflate, raw=added, before=added)[:3], (raw4, map4, s4), "adopt")
    # what ADD alone does with the same two clouds: the wall stays for ever
    assert mh.restate(room, 0.0, mh.CLAMP, base=added)[0][w].all()


def test_the_program_refuses_an_origin_outside_the_map(harness):
    import subprocess
    for origin in (sh.LOWER - 0.01, sh.UPPER.copy(), np.array([0.0, 0.0, 1.82]), np.array([np.nan, 0.0, 0.5])):
        with pytest.raises(subprocess.CalledProcessError) as e:
            sh.run(harness, np.zeros((1, 3), np.float32), origin, 1.0)
        assert e.value.returncode == 3
        assert sh.origin_voxel(origin, sh.DIMS, sh.RES, sh.LOWER, sh.UPPER) is None


def test_header_names_its_rules_and_the_abi_declares_the_calls():
    text = open(os.path.join(ROOT, "direct_amd", "csrc", "map_scan_math.h")).read()
    assert "DIRECT_MAPCLOUD_NO_CONTRACT" in text and "namespace mapscan" in text and "sqrt(" not in text
    from direct_amd import cluster
    assert {"direct_cluster_map_integrate_scan", "direct_cluster_get_scan_grid"} <= set(cluster.EXPORTS)
    head = open(os.path.join(ROOT, "include", "direct_cluster.h")).read()
    for word in ("DIRECT_SCAN_RESET", "DIRECT_SCAN_CONTINUE", "DIRECT_SCAN_ADOPT", "direct_map_scan_t", "log-odds", "Unknown space"):
        assert word in head
    assert C_sizeof_scan() == 8 * 11 + 4 * 6


def C_sizeof_scan():
    import ctypes as C
    from direct_amd import cluster
    return C.sizeof(cluster.MapScan)
