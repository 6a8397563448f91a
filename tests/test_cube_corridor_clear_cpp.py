"""direct_amd/csrc/cube_corridor_clear_math.h compiled by g++ -Wall -Werror (tests/cube_corridor_harness.py, floor-filled), without a GPU:
the floor table against NumPy, the clear call's corridors against the EXISTING harness on the thresholded map (the independent
witness: bit for bit the plain call on (D2 < min_d2) ? 1 : 0), the integer guarantee, named cases, and the cache's slot choice.
The map is tests/cube_corridor_harness.py's crafted map, the rows are the 40 of tests/corridor_lib.py."""
import functools

import numpy as np
import pytest

from direct_amd import abi
from tests import corridor_lib as lib
from tests import cube_corridor_clear_harness as cl
from tests import cube_corridor_harness as ch

KEYS = abi.CUBE_CORRIDOR_OUTPUTS
CAP = 40
same = functools.partial(lib.same, keys=KEYS)


@pytest.fixture(scope="module")
def clear(tmp_path_factory):
    return cl.build(tmp_path_factory.mktemp("cube_corridor_clear_cpp"))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("cube_corridor_clear_plain"))


@pytest.fixture(scope="module")
def world():
    grid = ch.crafted_map()
    d2 = cl.brute_d2(grid)
    assert int(grid.sum()) == 325 and int(d2.max()) == 146 and np.array_equal(d2 == 0, grid == 1)
    xyz, n = ch.pack_paths(lib.rows40(), CAP)
    return grid, d2, xyz, n


def seed_voxels(r):
    return np.rint((r["seeds"] - ch.LOWER) / ch.RES - 0.5).astype(int)


def test_floor_table_equals_numpy(clear, world):
    """1.  the table from the header's index arithmetic is the cumsum of (d2 < min_d2), entry for entry; one floor above the largest
    D2 counts everything; the neutral floors give the map's table"""
    grid, d2, _, _ = world
    for floor in (2, 4, 9, int(d2.max()) + 1):
        want = np.zeros(tuple(s + 1 for s in grid.shape), np.int64)
        want[1:, 1:, 1:] = (d2 < floor).cumsum(0).cumsum(1).cumsum(2)
        got = cl.table(clear, grid, d2, floor)
        assert np.array_equal(got, want), floor
        assert got[-1, -1, -1] == (d2 < floor).sum()
    assert cl.table(clear, grid, d2, int(d2.max()) + 1)[-1, -1, -1] == grid.size
    occupied = np.zeros(tuple(s + 1 for s in grid.shape), np.int64)
    occupied[1:, 1:, 1:] = (grid == 1).cumsum(0).cumsum(1).cumsum(2)
    for floor in (0, 1):
        assert np.array_equal(cl.table(clear, grid, np.full_like(d2, -7), floor), occupied)   # the field is not looked at


def test_equals_the_plain_harness_on_the_thresholded_map(clear, plain, world):
    """2.  every output, byte for byte, both walks, both dtypes; floor 1 is the existing harness on the map itself.  The figures of
    the batch (polytopes per batch, most in one row, rows that differ from the plain call's) are those recorded for this map."""
    grid, d2, xyz, n = world
    base = ch.corridors(plain, grid, xyz, n, seg_capacity=CAP)
    figures = {}
    for floor in (1, 2, 4, 9, int(d2.max()) + 1):
        on = grid if floor == 1 else cl.thresholded(d2, floor)
        for pop_back, dtype, p_max in ((True, np.float64, 6), (False, np.float64, 7), (True, np.float32, 7), (False, np.float32, 6)):
            want = ch.corridors(plain, on, xyz, n, pop_back=pop_back, seg_capacity=CAP, p_max=p_max, dtype=dtype)
            got = cl.corridors(clear, grid, d2, floor, xyz, n, pop_back=pop_back, seg_capacity=CAP, p_max=p_max, dtype=dtype)
            same(got, want)
            if pop_back and dtype == np.float64:
                assert (got["rtn"] == ch.OK).all()
                differ = sum(got["cube_idx"][b].tobytes() != base["cube_idx"][b].tobytes() for b in range(len(n)))
                figures[floor] = (int(got["n_seg"].sum()), int(got["n_seg"].max()), differ)
    print(figures)
    assert [figures[f] for f in (1, 2, 4, 9)] == [(144, 14, 0), (262, 23, 39), (292, 22, 39), (475, 33, 39)]


def test_the_guarantee_in_integers(clear, world):
    """3.  every voxel of every kept cube other than its seed voxel has d2 >= min_d2; not vacuous: at floor 4 at least half of the
    kept cubes are larger than one voxel"""
    grid, d2, xyz, n = world
    for floor in (2, 4, 9):
        r = cl.corridors(clear, grid, d2, floor, xyz, n, seg_capacity=CAP)
        checked, large = cl.guarantee(r["cube_idx"], r["n_seg"], seed_voxels(r), d2, floor)
        assert checked == r["n_seg"].sum()
        if floor == 4:
            print("floor 4: %d of %d kept cubes larger than one voxel" % (large, checked))
            assert (checked, large) == (292, 226) and 2 * large >= checked


def one(clear, world, floor, path, **kw):
    grid, d2, _, _ = world
    xyz, n = ch.pack_paths([path], CAP)
    return cl.corridors(clear, grid, d2, floor, xyz, n, **kw)


FACES = ((0, -1), (1, -1), (2, -1), (0, 1), (1, 1), (2, 1))


def slab(c, axis, side):
    """the slab one voxel beyond a face of cube c (lo xyz, hi xyz), as slices"""
    lo, hi = list(c[:3]), list(c[3:])
    lo[axis] = hi[axis] = (c[axis] - 1) if side < 0 else (c[3 + axis] + 1)
    return tuple(slice(lo[a], hi[a] + 1) for a in range(3))


def test_seed_below_the_floor_still_gets_a_cube(clear, world):
    """4a.  (4, 4, 4) inside the room is two voxels from two walls: below the floor 9, and so are its six face neighbours - the cube
    is the seed voxel alone, and its polytope is that voxel.  At floor 2 the same seed, no longer below, gets the room's interior
    without the voxels that touch a wall."""
    grid, d2, _, _ = world
    seed = np.array([4, 4, 4])
    assert 0 < d2[tuple(seed)] < 9
    for axis, side in FACES:
        v = seed.copy()
        v[axis] += side
        assert d2[tuple(v)] < 9
    r = one(clear, world, 9, [seed])
    assert r["rtn"][0] == ch.OK and r["n_seg"][0] == 1 and r["cube_idx"][0, 0].tolist() == [4, 4, 4, 4, 4, 4]
    lo, hi = seed * ch.RES + ch.LOWER, (seed + 1) * ch.RES + ch.LOWER
    assert np.allclose(r["planes"][0, 0, :, 3], [lo[0], lo[1], lo[2], -hi[2], -hi[1], -hi[0]], rtol=0, atol=1e-12)
    assert one(clear, world, 2, [seed])["cube_idx"][0, 0].tolist() == [4, 4, 4, 6, 6, 6]
    assert one(clear, world, 1, [seed])["cube_idx"][0, 0].tolist() == [3, 3, 3, 7, 7, 7]


def test_face_stopped_by_a_free_voxel_below_the_floor(clear, world):
    """4b.  from (20, 3, 3) the plain cube goes on where the cube of floor 4 has stopped: on a face where the two differ, the slab
    beyond the clear cube's face holds no occupied voxel but one that is below the floor"""
    grid, d2, _, _ = world
    c0 = one(clear, world, 1, [[20, 3, 3]])["cube_idx"][0, 0]
    c4 = one(clear, world, 4, [[20, 3, 3]])["cube_idx"][0, 0]
    assert (c4[:3] >= c0[:3]).all() and (c4[3:] <= c0[3:]).all()
    found = 0
    for axis, side in FACES:
        at = axis if side < 0 else 3 + axis
        if c4[at] == c0[at]:
            continue
        s = slab(c4, axis, side)
        if not grid[s].any():
            assert (d2[s] < 4).any()
            found += 1
    assert found >= 1


def test_the_one_voxel_tunnel_at_floor_2(clear, world):
    """4c.  every voxel of the tunnel touches its walls (D2 = 1): at floor 2 each is below the floor, none may enter another's cube,
    and the path through the tunnel gets a polytope per tunnel voxel, where the plain call covers tunnel and exit with one.  All are
    one voxel but the last: the voxels beyond the open end have D2 >= 2, and the cube of the tunnel's last voxel (whose own D2 is
    not looked at) grows out through them to the border."""
    grid, d2, _, _ = world
    path = next(c for c in ch.named_cases() if c["name"] == "thin_corridor")["paths"][0]
    tunnel = [p for p in path if 11 <= p[0] <= 20]
    assert len(tunnel) == 9 and all(d2[tuple(p)] == 1 for p in tunnel) and all(d2[x, 12, 5] >= 2 for x in (21, 22, 23))
    r0, r2 = one(clear, world, 1, path), one(clear, world, 2, path)
    assert r0["n_seg"][0] == 1 and r0["cube_idx"][0, 0].tolist() == [11, 12, 5, 23, 12, 5]
    assert r2["n_seg"][0] == len(tunnel)
    assert r2["cube_idx"][0, :len(tunnel)].tolist() == [list(p) + list(p) for p in tunnel[:-1]] + [[20, 12, 5, 23, 12, 5]]


def test_seg_capacity_32_at_floor_9(clear, world):
    """4d.  exactly one OVERFLOW row, its n_seg the number needed, the kept polytopes those of the full call"""
    grid, d2, xyz, n = world
    full = cl.corridors(clear, grid, d2, 9, xyz, n, seg_capacity=CAP)
    cut = cl.corridors(clear, grid, d2, 9, xyz, n, seg_capacity=32)
    over = np.flatnonzero(cut["rtn"] == ch.OVERFLOW)
    assert len(over) == 1 and (np.delete(cut["rtn"], over) == ch.OK).all()
    assert np.array_equal(cut["n_seg"], full["n_seg"]) and cut["n_seg"][over[0]] == 33
    for k in ("n_planes", "planes", "seeds", "centers", "cube_idx"):
        assert np.array_equal(cut[k], full[k][:, :32]), k


def test_slot_choice(tmp_path):
    """5.  hit, miss into an empty slot, the least recently used as victim, and a changed serial never hitting - the function alone,
    as a stand-alone program"""
    exe = cl.build_slots(tmp_path)
    assert abi.CUBE_CORRIDOR_FLOOR_SLOTS == 2
    # the floors 4, 4, 9, 4, 16, 4, 9 on one field: builds 1, 0, 1, 0, 1, 0, 1
    got = cl.slot_choices(exe, [(f, 1) for f in (4, 4, 9, 4, 16, 4, 9)])
    assert [1 - hit for _, hit in got] == [1, 0, 1, 0, 1, 0, 1]
    assert [s for s, _ in got] == [0, 0, 1, 0, 1, 0, 1]          # empty slots in order, then 9 and 16 take turns beside 4
    # two floors alternating never rebuild
    assert [hit for _, hit in cl.slot_choices(exe, [(4, 1), (9, 1)] * 4)] == [0, 0] + [1] * 6
    # the least recently used goes, not the oldest build
    assert cl.slot_choices(exe, [(4, 1), (9, 1), (4, 1), (16, 1), (4, 1), (9, 1)]) == [(0, 0), (1, 0), (0, 1), (1, 0), (0, 1), (1, 0)]
    assert cl.slot_choices(exe, [(4, 1), (9, 1), (16, 1), (9, 1), (4, 1)]) == [(0, 0), (1, 0), (0, 0), (1, 1), (0, 0)]
    # a changed serial never hits, and the same floor on the new field does again
    assert cl.slot_choices(exe, [(4, 1), (9, 1), (4, 2), (4, 2), (9, 2), (9, 2)]) == [(0, 0), (1, 0), (0, 0), (0, 1), (1, 0), (1, 1)]
