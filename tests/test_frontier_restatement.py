"""Known space and frontier goals without a GPU: the g++ build of map_scan_math.h, free_comp_math.h and frontier_math.h
(tests/frontier_harness.py, one stand-alone program that emulates the kernels as lane loops) against the NumPy restatement written
from the definition's text.  Everything is bytes, indices and counts: every comparison is for equality."""
import ctypes as C

import numpy as np
import pytest

from direct_amd import cluster
from tests import dist_field_harness as dh
from tests import free_comp_harness as fh
from tests import frontier_harness as fr
from tests import map_scan_harness as sh


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return fr.build(str(tmp_path_factory.mktemp("frontier")))


_KNOWN, _COMP = {}, {}


def known_of(name, r):
    """the restated known grid of one tracked scan of a cloud from an empty grid, computed once"""
    if (name, r) not in _KNOWN:
        _KNOWN[name, r] = fr.known_restate(sh.clouds()[name], sh.ORIGIN, r)
    return _KNOWN[name, r]


def comp_of(name):
    if name not in _COMP:
        grid, known = {n: (g, k) for n, g, k in fr.scenes()}[name]
        _COMP[name] = (grid, known, fr.components(grid, known))
    return _COMP[name]


SCENES = [n for n, _, _ in fr.scenes()]


# ---- the known grid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sh.clouds()))
def test_known_grid_of_every_cloud(exe, name):
    """RESET on a handle that held a full known grid, at the three ranges, with the carve's two store choices; the scan grid and the
    stats are those of the untracked scan"""
    pts = sh.clouds()[name]
    full = np.ones(sh.DIMS, np.uint8)
    for r in sh.RANGES:
        want = known_of(name, r)
        raw, _, stats = sh.restate(pts, sh.ORIGIN, r)
        for test_store in (True, False):
            got = fr.run_scan(exe, pts, sh.ORIGIN, r, mode=fr.RESET, known=full, test_store=test_store)
            assert np.array_equal(got["known"], want), (name, r, test_store, int((got["known"] != want).sum()))
            assert np.array_equal(got["raw"], raw) and got["stats"].tolist() == stats[:4].tolist()
            plain = fr.run_scan(exe, pts, sh.ORIGIN, r, mode=fr.RESET, flags=0, known=full, test_store=test_store)
            assert plain["known"] is None and np.array_equal(plain["raw"], raw) and plain["stats"].tolist() == stats[:4].tolist()
        assert name == "nonfinite" or want.any()
        # every ray that contributes anything passes the origin's voxel, or ends in it
        assert bool(want[tuple(sh.origin_voxel(sh.ORIGIN, sh.DIMS, sh.RES, sh.LOWER, sh.UPPER))]) == bool(want.any())


def test_known_grid_modes(exe):
    clouds = sh.clouds()
    a, b = clouds["random"][:500], clouds["lattice"]
    ka, kb = fr.known_restate(a, sh.ORIGIN, 1.5), fr.known_restate(b, sh.ORIGIN, 10.0)
    # CONTINUE on a handle without a known grid starts empty; a second scan gives the union
    s1 = fr.run_scan(exe, a, sh.ORIGIN, 1.5, mode=fr.CONTINUE)
    assert np.array_equal(s1["known"], ka)
    s2 = fr.run_scan(exe, b, sh.ORIGIN, 10.0, mode=fr.CONTINUE, raw=s1["raw"], known=s1["known"])
    assert np.array_equal(s2["known"], ka | kb) and (ka | kb).sum() > max(ka.sum(), kb.sum())
    assert np.array_equal(s2["known"], fr.known_restate(b, sh.ORIGIN, 10.0, known=ka))
    # ADOPT takes the map's bytes as the scan grid and keeps the known grid
    full = np.ones(sh.DIMS, np.uint8)
    s3 = fr.run_scan(exe, a, sh.ORIGIN, 1.5, mode=fr.ADOPT, raw=full, known=s2["known"])
    assert np.array_equal(s3["known"], ka | kb)
    assert np.array_equal(s3["raw"], sh.restate(a, sh.ORIGIN, 1.5, raw=full)[0])
    # RESET empties it
    s4 = fr.run_scan(exe, a, sh.ORIGIN, 1.5, mode=fr.RESET, raw=s3["raw"], known=s3["known"])
    assert np.array_equal(s4["known"], ka)
    # an untracked scan in between drops the grid: the next tracked CONTINUE starts empty
    s5 = fr.run_scan(exe, b, sh.ORIGIN, 10.0, mode=fr.CONTINUE, flags=0, raw=s4["raw"], known=s4["known"])
    assert s5["known"] is None
    s6 = fr.run_scan(exe, a, sh.ORIGIN, 1.5, mode=fr.CONTINUE, raw=s5["raw"], known=s5["known"])
    assert np.array_equal(s6["known"], ka)
    # any other flag bit is refused
    for flags in (2, 3, -1, 1 << 30):
        assert fr.run_scan(exe, a, sh.ORIGIN, 1.5, flags=flags) == 1


def test_known_grid_does_not_depend_on_the_order_of_the_points(exe):
    pts = np.concatenate(list(sh.clouds().values()))
    first = fr.run_scan(exe, pts, sh.ORIGIN, 1.5)
    for variant in (pts[::-1], pts[np.random.default_rng(3).permutation(len(pts))]):
        got = fr.run_scan(exe, variant, sh.ORIGIN, 1.5)
        assert got["known"].tobytes() == first["known"].tobytes() and got["raw"].tobytes() == first["raw"].tobytes()


def test_binding_follows_the_rename():
    assert [n for n, _ in cluster.MapScan._fields_][-3:] == ["mode", "stride", "flags"]
    assert cluster.MapScan.flags.offset == 108 and C.sizeof(cluster.MapScan) == 112 and cluster.SCAN_TRACK_KNOWN == 1
    for method in ("known_grid", "set_known", "frontiers"):
        assert callable(getattr(cluster.ClusterGenerator, method))


# ---- the frontier -------------------------------------------------------------------------------------------------------------
def spans_two_tiles_in_each_axis(label):
    for r in np.unique(label[label >= 0]):
        vox = np.argwhere(label == r)
        if all(len(np.unique(vox[:, a] // 8)) >= 2 for a in range(3)):
            return True
    return False


def test_the_restatement_is_not_empty():
    """what the comparison below would otherwise pass on silently"""
    comps = {n: comp_of(n)[2] for n in SCENES}
    assert any(len(c["roots"]) >= 8 for c in comps.values())
    assert any(fh.spans_tiles(c["label"]) >= 1 and spans_two_tiles_in_each_axis(c["label"]) for c in comps.values())
    assert any(r["tie"] for c in comps.values() for r in c["roots"])
    assert any(not r["centroid_member"] for c in comps.values() for r in c["roots"])
    board = comps["checkerboard"]["roots"]
    assert sum(r["size"] == 1 for r in board) >= 8 and sum(r["size"] == 3 and r["tie"] and not r["centroid_member"] for r in board) >= 8
    ball = comps["ball"]
    assert len(ball["roots"]) == 1 and not ball["roots"][0]["centroid_member"]
    # the map border is not a frontier: no frontier voxel of the box lies on its three map faces alone
    box = comps["box_on_three_faces"]["front"]
    assert box.any() and not box[0, 0, 0] and not box[0, :5, :3].any()
    # every representative is known, enterable and on the frontier
    for n in SCENES:
        grid, known, c = comp_of(n)
        for r in c["roots"]:
            assert c["front"][r["rep"]] and known[r["rep"]] != 0 and grid[r["rep"]] == 0 and c["label"][r["rep"]] == r["label"]


@pytest.mark.parametrize("name", SCENES)
def test_frontier_equals_the_restatement(exe, name):
    grid, known, comp = comp_of(name)
    sizes = sorted(r["size"] for r in comp["roots"])
    mid = sizes[len(sizes) // 2]
    kept = len(sizes)
    for min_size in sorted({1, mid, mid + 1, sizes[-1], sizes[-1] + 1}):       # below, at and above a component's size
        want = fr.select(comp, min_size, 1024)
        fr.assert_same(fr.run_frontier(exe, grid, known, min_size=min_size), want, (name, min_size))
        assert (min_size <= sizes[-1]) == (want["stats"][3] > 0)
    for cap in sorted({0, max(kept - 1, 0), kept, kept + 3}):                  # none, below, at and above kept
        want = fr.select(comp, 1, cap)
        fr.assert_same(fr.run_frontier(exe, grid, known, capacity=cap), want, (name, cap))
        assert want["stats"][4] == min(cap, kept) and want["stats"][3] == kept


@pytest.mark.parametrize("width", (3, 5))
def test_frontier_with_a_floor(exe, width):
    grid, known = fr.door_scene(width)
    d2 = dh.brute_d2(grid)
    floor = fh.separating_floor(grid, d2)
    plain = fr.components(grid, known)
    for min_d2 in (2, floor, floor + 5):
        comp = fr.components(grid, known, d2, min_d2)
        assert 0 < comp["front"].sum() < plain["front"].sum()            # the frontier draws back from the wall
        assert len(comp["roots"]) == (2 if min_d2 >= floor else 1) and len(plain["roots"]) == 1
        for min_size, cap in ((1, 1024), (5, 1024), (1, 0), (1, 1)):
            got = fr.run_frontier(exe, grid, known, d2, min_d2, min_size, cap)
            fr.assert_same(got, fr.select(comp, min_size, cap), (width, min_d2, min_size, cap))
    fr.assert_same(fr.run_frontier(exe, grid, known, None, 1), fr.select(plain), "min_d2 = 1 is the graph without a floor")


def test_the_scan_crosses_a_lane_s_run(exe):
    """40 x 36 x 20 voxels are 113 workgroup counts: two words per lane of the exclusive scan"""
    grid = (np.random.default_rng(5).random(fh.DIMS_BIG) < 0.2).astype(np.uint8)
    known = (np.random.default_rng(6).random(fh.DIMS_BIG) < 0.05).astype(np.uint8)
    comp = fr.components(grid, known)
    assert len(comp["roots"]) > 113
    for min_size, cap in ((1, 4096), (3, 4096), (1, 200)):
        fr.assert_same(fr.run_frontier(exe, grid, known, min_size=min_size, capacity=cap), fr.select(comp, min_size, cap), (min_size, cap))


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: one tracked scan in each store mode and two frontier calls"""
    san = fr.build(str(tmp_path), sanitize=True)
    pts = np.concatenate(list(sh.clouds().values()))
    for test_store in (True, False):
        got = fr.run_scan(san, pts, sh.ORIGIN, 10.0, mode=fr.RESET, test_store=test_store)
        assert got["known"].any()
    for name in ("ball", "checkerboard"):
        grid, known, comp = comp_of(name)
        fr.assert_same(fr.run_frontier(san, grid, known, min_size=2, capacity=7), fr.select(comp, 2, 7), name)
