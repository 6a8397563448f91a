"""direct_amd/csrc/free_comp_math.h, compiled by g++ and run as the kernels run it (tests/free_comp_harness.py), against an
independent NumPy restatement: brute-force D2, a stack flood fill over 26 neighbours, label = smallest index, sizes by counting;
pairs against a flood fill from the start's neighbours.  No GPU."""
import numpy as np
import pytest

from tests import dist_field_harness as dh
from tests import free_comp_harness as fh


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return fh.build(tmp_path_factory.mktemp("free_comp"))


def hold(exe, grid, d2=None, min_d2=0, what=""):
    want = fh.restate(grid, d2, min_d2)
    got = fh.run(exe, grid, d2, min_d2)
    fh.assert_same(got, *want, what=what)
    return want


def test_named_maps(exe):
    """1.  the crafted maps on 24 x 20 x 12: what each must give is asserted from the restatement first, then the header is held
    to it"""
    expect = {"empty": (5760, 1, 5760, 0), "full": (0, 0, 0, -1), "checkerboard": (2880, 1, 2880, 0), "even_lattice": (720, 720, 1, 0),
              "corner_3_borders": (2, 1, 2, (7 * 20 + 7) * 12 + 7), "edge_diagonal": (2, 1, 2, (7 * 20 + 7) * 12 + 3)}
    for name, grid in fh.named_maps():
        label, size, stats = hold(exe, grid, what=name)
        if name in expect:
            assert tuple(stats) == expect[name], (name, stats)
        if name == "full":
            assert (label == -1).all() and (size == 0).all()
        if name == "serpentine":
            assert stats[1] == 1 and stats[3] == 0 and fh.spans_tiles(label) == 1
            xs, ys, zs = np.nonzero(label >= 0)
            assert len(set(zip(xs // 8, ys // 8, zs // 8))) == 18   # every tile
        if name == "far_end":
            assert stats[1] == 1 and stats[3] == 1 * 12 + 1 and label[1, 5, 1] == label[0, 1, 1] == 13 and grid[0, 5, 1] == 1
        if name == "byte_2":
            assert (label[10:14] == -1).all() and stats[1] == 2 and label[9, 0, 0] == 1 and label[14, 0, 0] == 14 * 240
            # a byte of 2 is no obstacle for D2: with a floor the slab's neighbours stay enterable
            d2 = dh.brute_d2(grid)
            assert d2[12, 5, 5] > 100 and d2[9, 10, 6] >= 4
            hold(exe, grid, d2, 4, what="byte_2 floor 4")


def test_degenerate_sizes(exe):
    """2."""
    for name, grid in fh.degenerate_maps():
        label, size, stats = hold(exe, grid, what=name)
        if name == "1024x2x2":
            assert tuple(stats) == (4096, 1, 4096, 0)   # one chain across 128 tiles


@pytest.mark.parametrize("name,grid", fh.random_maps(), ids=[n for n, _ in fh.random_maps()])
def test_random_maps(exe, name, grid):
    """3.  12 % free: many components, at least 10 of them across tile borders, and sampled pairs of both kinds"""
    label, size, stats = fh.restate(grid)
    assert fh.spans_tiles(label) >= 10, fh.spans_tiles(label)
    starts, goals = fh.free_pairs(grid, 200, 11)
    want = np.where(label[tuple(starts.T)] == label[tuple(goals.T)], fh.OK, fh.NO_PATH)
    assert (want == fh.OK).mean() >= 0.2 and (want == fh.NO_PATH).mean() >= 0.2, (want == fh.OK).mean()
    got = fh.run(exe, grid, starts=starts, goals=goals)
    fh.assert_same(got, label, size, stats, what=name)
    assert np.array_equal(got["rtn"], want)
    assert np.array_equal(got["goal_label"], label[tuple(goals.T)]) and np.array_equal(got["goal_size"], size[tuple(goals.T)])
    print("%s: %d components, %d across tiles, %.0f %% of pairs connected, %d cross-tile unions"
          % (name, stats[1], fh.spans_tiles(label), 100 * (want == fh.OK).mean(), got["unions"]))


@pytest.mark.parametrize("width", [1, 3, 5])
def test_floors(exe, width):
    """5.  a wall with one door: the smallest floor at which the rooms separate comes from the restatement; the header is held to it
    at that floor and the one below, on the uncapped and on a capped field; a floor above cap2 is refused"""
    grid = fh.door_map(width)
    d2 = dh.brute_d2(grid)
    floor = fh.separating_floor(grid, d2)
    assert floor == {1: 2, 3: 5, 5: 10}[width]
    counts = [fh.restate(grid, d2, f)[2][1] for f in (floor - 1, floor)]
    assert counts[0] != counts[1], counts
    cap_vox = 4
    capped = dh.brute_d2(grid, cap_vox)
    assert capped.max() == cap_vox * cap_vox and floor <= cap_vox * cap_vox
    for f in (floor - 1, floor):
        want = hold(exe, grid, d2, f, what="door %d floor %d" % (width, f))
        got = fh.run(exe, grid, capped, f, cap2=cap_vox * cap_vox)
        fh.assert_same(got, *want, what="capped")   # below cap2 the capped field says what the exact one says
    assert fh.run(exe, grid, capped, cap_vox * cap_vox + 1, cap2=cap_vox * cap_vox) is None
    assert fh.run(exe, grid, capped, cap_vox * cap_vox, cap2=cap_vox * cap_vox) is not None


def test_pair_rule(exe):
    """6.  occupied starts, s == g on an occupied voxel, a goal beside an occupied start, endpoints outside on each side: the codes
    are those of a flood fill from the start's neighbours, which uses no labels"""
    grid = fh.random_map(fh.DIMS, 1)
    starts, goals = fh.rule_pairs(grid)
    want = fh.witness_codes(grid, starts, goals)
    assert (want == fh.BAD_ENDPOINT).sum() == 12 and want[16] == fh.OK and grid[tuple(starts[16])] == 1 and want[17] == fh.OK
    assert (grid[tuple(starts[:16].T)] == 1).all() and {fh.OK, fh.NO_PATH} <= set(want[:16].tolist())
    label, size, _ = fh.restate(grid)
    got = fh.run(exe, grid, starts=starts, goals=goals)
    assert np.array_equal(got["rtn"], want), (got["rtn"], want)
    inside = ((goals >= 0) & (goals < np.array(grid.shape))).all(1)
    gl = np.where(inside, label[tuple(np.clip(goals, 0, np.array(grid.shape) - 1).T)], -1)
    gs = np.where(inside, size[tuple(np.clip(goals, 0, np.array(grid.shape) - 1).T)], 0)
    assert np.array_equal(got["goal_label"], gl) and np.array_equal(got["goal_size"], gs)
    # the same rule under a floor, on a door map: starts below the floor leave through a neighbour that is not
    door = fh.door_map(3)
    d2 = dh.brute_d2(door)
    s2, g2 = fh.free_pairs(door, 48, 3)
    s2[:12] = np.argwhere((door == 0) & (d2 < 5))[:12]
    for f in (4, 5):
        assert np.array_equal(fh.run(exe, door, d2, f, starts=s2, goals=g2)["rtn"], fh.witness_codes(door, s2, g2, d2, f)), f
