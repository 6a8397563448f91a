"""Visible unknown volume per candidate viewpoint without a GPU: the g++ build of view_gain_math.h (tests/view_gain_harness.py, one
stand-alone program that emulates the workgroup as a lane loop with the box of bits) against the restatement in Python floats
written from the definition's text, and the identities the definition implies.  The outputs are counts: every comparison is for
equality."""
import math

import numpy as np
import pytest

from tests import map_scan_harness as sh
from tests import view_gain_harness as vh


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return vh.build(str(tmp_path_factory.mktemp("view_gain")))


DIRSETS = dict(sign=vh.dirs_sign, random=lambda: vh.dirs_random(400), degenerate=vh.dirs_degenerate)
RANGES = (0.3, 3.49, 10.0)


def check_offsets(out, range_vox):
    """the largest offset reached is at most floor(range_vox + 0.5), which is at most R - 1: the visited set fits the box"""
    top = int(math.floor(range_vox + 0.5))
    assert top <= vh.box_half(range_vox) - 1
    assert (out["max_offset"] <= top).all(), (range_vox, out["max_offset"].max())


@pytest.mark.parametrize("scene", sorted(vh.scenes()))
@pytest.mark.parametrize("dirset", sorted(DIRSETS))
def test_program_equals_the_restatement(exe, scene, dirset):
    grid, known = vh.scenes()[scene]
    cand, dirs = vh.candidates(grid), DIRSETS[dirset]()
    for r in RANGES:
        want = vh.restate(grid, known, cand, dirs, r)
        got = vh.run(exe, grid, known, cand, dirs, r, lanes=64)
        vh.assert_same(got, want, (scene, dirset, r))
        assert np.array_equal(got["max_offset"], want["max_offset"])
        check_offsets(got, r)
        ok = want["code"] == vh.OK
        assert ok.any() and (want["code"] == vh.OUTSIDE).sum() >= 6
        assert (want["ends"].sum(axis=1) == np.where(ok, len(dirs), 0)).all()            # every ray of an OK candidate ends once
        assert (want["seen"][ok] >= 1).all() or dirset == "degenerate"
        assert not want["gain"][~ok].any() and not want["seen"][~ok].any() and not want["ends"][~ok].any()
        if scene == "empty_unknown":
            assert np.array_equal(got["gain"], got["seen"])
        if scene == "empty_known":
            assert not got["gain"].any()
        if scene.startswith("empty"):
            assert not got["ends"][:, vh.BLOCKED].any()
    if scene == "random":
        assert (want["code"] == vh.OCCUPIED).any() and want["ends"][:, vh.BLOCKED].any() and want["ends"][:, vh.LEFT].any()
    if dirset == "degenerate":
        assert (want["ends"][ok, vh.SKIPPED] == 7).all()   # five rows with a NaN or an infinity, the zero row, the signed-zero row


def test_sets_and_bad_set_indices(exe):
    grid, known = vh.scenes()["random"]
    cand = vh.candidates(grid)
    sets_dirs = np.stack([vh.dirs_random(26, seed=s) for s in (1, 2)] + [vh.dirs_sign()])
    sets = np.array([(c % 5) - 1 for c in range(len(cand))], np.int32)      # -1 and 3 are outside [0, 3)
    want = vh.restate(grid, known, cand, sets_dirs, 5.5, sets)
    got = vh.run(exe, grid, known, cand, sets_dirs, 5.5, sets)
    vh.assert_same(got, want)
    assert (want["code"] == vh.BAD_SET).any() and {int(s) for s, c in zip(sets, want["code"]) if c == vh.OK} == {0, 1, 2}
    for s in range(3):                                                        # a set of a stacked call is that set alone
        alone = vh.run(exe, grid, known, cand[sets == s], sets_dirs[s], 5.5)
        for k in vh.KEYS:
            assert np.array_equal(alone[k], got[k][sets == s]), (s, k)


@pytest.mark.parametrize("range_vox", (0.3, 0.5, 2.6, 3.49, 3.5, 7.0))
def test_axis_rays_on_an_empty_map(exe, range_vox):
    """a voxel at offset k along an axis is entered at distance k - 1/2: seen == 1 + 6 * floor(range_vox + 0.5)"""
    grid = np.zeros((20, 20, 20), np.uint8)
    cand = np.array([(10, 10, 10), (9, 10, 9)], np.int32)
    assert vh.box_half(range_vox) <= 9
    want = vh.restate(grid, grid, cand, vh.dirs_axis(), range_vox)
    got = vh.run(exe, grid, grid, cand, vh.dirs_axis(), range_vox, lanes=4)
    vh.assert_same(got, want)
    k = int(math.floor(range_vox + 0.5))
    assert got["seen"].tolist() == [1 + 6 * k] * 2 and got["gain"].tolist() == [1 + 6 * k] * 2
    assert got["ends"].tolist() == [[0, 0, 6, 0]] * 2 and got["max_offset"].tolist() == [k, k]


def test_the_largest_offsets_of_long_ranges(exe):
    """random, diagonal and axis directions on an empty map wider than the box, up to the largest supported range"""
    grid = np.zeros((101, 101, 101), np.uint8)
    cand = np.array([(50, 50, 50)], np.int32)
    dirs = np.concatenate([vh.dirs_sign(), vh.dirs_random(300, seed=11)])
    for r in (20.5, 47.5, 48.0, 48.99):
        got = vh.run(exe, grid, grid, cand, dirs, r)
        check_offsets(got, r)
        assert got["max_offset"][0] == int(math.floor(r + 0.5)) and got["ends"][0].tolist() == [0, 0, len(dirs), 0]
    want = vh.restate(grid, grid, cand, dirs, 48.99)
    vh.assert_same(got, want)


def test_translation_by_whole_voxels(exe):
    """the random scene inside a larger random map, three, two and one voxels in: candidates whose box of reach (offsets up to
    floor(range_vox + 0.5)) stays inside the scene see the same voxels"""
    grid, known = vh.scenes()["random"]
    shift, r = np.array([3, 2, 1]), 3.5
    rng = np.random.default_rng(5)
    big = tuple(int(d) + 2 * int(s) for d, s in zip(grid.shape, shift))
    grid2, known2 = (rng.random(big) < 0.2).astype(np.uint8), (rng.random(big) < 0.5).astype(np.uint8)
    inner = tuple(slice(int(s), int(s) + d) for s, d in zip(shift, grid.shape))
    grid2[inner], known2[inner] = grid, known
    reach = int(math.floor(r + 0.5))
    free = np.argwhere(grid == 0)
    free = free[np.all((free >= reach) & (free < np.array(grid.shape) - reach), axis=1)]
    cand = free[np.random.default_rng(6).choice(len(free), 12, replace=False)].astype(np.int32)
    dirs = np.concatenate([vh.dirs_sign(), vh.dirs_random(100, seed=12)])
    a = vh.run(exe, grid, known, cand, dirs, r)
    b = vh.run(exe, grid2, known2, cand + shift.astype(np.int32), dirs, r)
    for k in vh.KEYS + ("max_offset",):
        assert np.array_equal(a[k], b[k]), k
    assert a["seen"].min() > 1 and not a["ends"][:, vh.LEFT].any()
    vh.assert_same(a, vh.restate(grid, known, cand, dirs, r))


def test_permuting_directions_and_candidates(exe):
    grid, known = vh.scenes()["wall_and_room"]
    cand = vh.candidates(grid, n_free=10)
    dirs = np.concatenate([vh.dirs_sign(), vh.dirs_random(100, seed=13), vh.dirs_degenerate()])
    base = vh.run(exe, grid, known, cand, dirs, 10.0, lanes=256)
    pd, pc = np.random.default_rng(1).permutation(len(dirs)), np.random.default_rng(2).permutation(len(cand))
    for lanes in (1, 7, 64):                                                  # ... nor does the launch shape matter
        shuffled = vh.run(exe, grid, known, cand, dirs[pd], 10.0, lanes=lanes)
        moved = vh.run(exe, grid, known, cand[pc], dirs, 10.0, lanes=lanes)
        for k in vh.KEYS:
            assert np.array_equal(shuffled[k], base[k]) and np.array_equal(moved[k], base[k][pc]), (k, lanes)
    assert base["ends"][:, vh.BLOCKED].any() and (base["gain"] > 0).any() and (base["gain"] < base["seen"]).any()


def test_the_ideal_scan_identity():
    """the voxels the carve of map_integrate_scan clears for the points centre + 64 * dir on an empty dyadic grid are the seen set
    at range_vox = max_range / resolution: the gain IS the growth of the known grid under an ideal scan"""
    D = vh.DYADIC
    dirs = vh.dirs_dyadic()
    pts, centre = vh.dyadic_cloud(dirs)
    grid = np.zeros(D["dims"], np.uint8)
    assert tuple(sh.origin_voxel(centre, D["dims"], D["res"], D["lower"], D["upper"])) == D["v0"]
    sizes = []
    for max_range in vh.DYADIC_RANGES:
        cleared = set()
        for p in pts:
            cleared.update(sh.walk(p, centre, max_range, D["dims"], D["res"], D["lower"], D["upper"])[1])
        got = vh.restate(grid, grid, [D["v0"]], dirs, max_range / D["res"])
        assert got["visited"][0] == cleared, (max_range, len(cleared), got["seen"][0])
        sizes.append(len(cleared))
    assert sizes == sorted(sizes) and sizes[0] > 100 and sizes[-1] > 3000


def test_the_sanitized_program_on_the_random_scene(tmp_path):
    exe = vh.build(str(tmp_path), sanitize=True)
    grid, known = vh.scenes()["random"]
    cand = vh.candidates(grid)
    dirs = np.concatenate([vh.dirs_sign(), vh.dirs_random(400), vh.dirs_degenerate()])
    for r in (0.3, 10.0, 48.99):
        vh.assert_same(vh.run(exe, grid, known, cand, dirs, r), vh.restate(grid, known, cand, dirs, r), r)


def test_unsupported_ranges_are_refused_by_the_program(exe):
    """floor(range_vox) + 2 > 50: the program exits with status 3 before it sizes a box"""
    grid = np.zeros((4, 4, 4), np.uint8)
    for r, ok in ((48.99, True), (49.0, False), (1e300, False)):
        try:
            vh.run(exe, grid, grid, [(1, 1, 1)], vh.dirs_axis(), r)
            ran = True
        except AssertionError as e:
            ran = False
            assert e.args[0][0] == 3
        assert ran == ok, r
