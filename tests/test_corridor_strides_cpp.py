"""The inputs of tests/corridor_stride_lib.py on the CPU harnesses: each is built so that a strided loop of the corridor kernels
(direct_amd/csrc/cluster_corridor.h, cube_corridor.h) takes a second trip, and each test here asserts THAT PROPERTY on the g++
build of the rule headers and the CPU oracles - more than 64 planes deciding a plane test, more than 64 points, more than 64
polytopes, an owner across row 1024, more than 524288 slots.  An input that stops reaching its path fails here, without a GPU;
tests/test_gpu_corridor_strides.py then holds the device against the same harness results."""
import subprocess

import numpy as np
import pytest

from tests import corridor_lib as lib
from tests import corridor_stride_lib as sl
from tests import cube_corridor_clear_harness as cl
from tests import cube_corridor_harness as ch
from tests import cluster_corridor_harness as kh

WALK = ("n_seg", "seeds", "centers", "rtn")   # what the walk decides; planes and n_planes of a cut table differ by construction
CUBE_KEYS = ("n_seg", "n_planes", "planes", "seeds", "centers", "cube_idx", "rtn")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return sl.build_harness("cluster", tmp_path_factory)


@pytest.fixture(scope="module")
def cube_harness(tmp_path_factory):
    return sl.build_harness("cube", tmp_path_factory)


@pytest.fixture(scope="module")
def clear_harness(tmp_path_factory):
    return sl.build_harness("clear", tmp_path_factory)


# ---- 1. polytopes over 64 planes in the walk ----------------------------------------------------------------------------------

@pytest.mark.parametrize("pop_back", [True, False])
def test_planes_of_index_64_and_above_decide(harness, pop_back):
    """every row OK and equal to oracle.corridor_walk; polytopes of more than 64 planes, two of them in one row's stack; pops under
    pop_back.  The MUTANT - every polytope cut to its first 64 planes - walks differently (n_seg, seeds, centres or codes) or asks
    for a seed the real walk never asks for (status 3): a plane of index 64 or above alone decides a test.  This holds for BOTH
    pop settings: without pop, through the two rows of wide_rows() that end at a voxel only such planes exclude."""
    rows = sl.wide_rows()
    want, table = kh.oracle_corridors(rows, sl.WIDE_ITR, pop_back, grid=sl.two_ball_map(), tag="two_balls")
    xyz, n = ch.pack_paths(rows, sl.WIDE_CAP)
    got = kh.corridors(harness, xyz, n, table, pop_back=pop_back, seg_capacity=sl.WIDE_SEG, p_max=sl.WIDE_PMAX)
    assert (got["rtn"] == kh.OK).all()
    kh.assert_rows_equal_oracle(got, want, rows)
    wide_per_row = (got["n_planes"] > 64).sum(1)
    print("pop %d: max planes %d, most wide polytopes in a row %d, stats %s" % (pop_back, got["n_planes"].max(), wide_per_row.max(), got["stats"]))
    assert int((sl.two_ball_map() == 0).sum()) == 1436
    assert 64 < got["n_planes"].max() <= sl.WIDE_PMAX and wide_per_row.max() >= 2
    assert (got["stats"]["pops"] > 0) == pop_back
    try:
        cut = kh.corridors(harness, xyz, n, sl.cut_table(table), pop_back=pop_back, seg_capacity=sl.WIDE_SEG, p_max=sl.WIDE_PMAX)
    except subprocess.CalledProcessError as e:
        assert e.returncode == 3
    else:
        assert any(cut[k].tobytes() != got[k].tobytes() for k in WALK)


def test_p_max_64_stops_rows_at_their_first_wide_polytope(harness):
    """p_max = 64: a row stops TOO_MANY_PLANES at its first polytope of more than 64 planes with the head of its corridor; both
    kinds of row occur"""
    rows = sl.wide_rows()
    _, table = kh.oracle_corridors(rows, sl.WIDE_ITR, False, grid=sl.two_ball_map(), tag="two_balls")
    xyz, n = ch.pack_paths(rows, sl.WIDE_CAP)
    full = kh.corridors(harness, xyz, n, table, pop_back=False, seg_capacity=sl.WIDE_SEG, p_max=sl.WIDE_PMAX)
    few = kh.corridors(harness, xyz, n, table, pop_back=False, seg_capacity=sl.WIDE_SEG, p_max=64)
    assert sl.stopped_at_first_wide(few, full, 64) not in (0, len(rows))


# ---- 2. paths over 64 points ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pop_back", [True, False])
def test_long_paths_cluster(harness, pop_back):
    """rows of 64, 65, 128, 129 and 150 points at a path capacity of 150: equal to oracle.corridor_walk; the points from index 64 on
    matter (the rows cut to 64 points give other corridors); at seg_capacity 260 everything behind n_seg is zero up to slot 259"""
    rows = sl.long_rows()
    assert {64, 65, 128, 129, 150} <= {len(r) for r in rows} and sl.LONG_CAP % 64
    want, table = kh.oracle_corridors(rows, sl.BIG_ITR, pop_back)
    xyz, n = ch.pack_paths(rows, sl.LONG_CAP)
    got = kh.corridors(harness, xyz, n, table, pop_back=pop_back, seg_capacity=sl.LONG_CAP, p_max=sl.BIG_PMAX)
    assert (got["rtn"] == kh.OK).all() and got["n_planes"].max() <= sl.BIG_PMAX
    kh.assert_rows_equal_oracle(got, want, rows)
    hx, hn = ch.pack_paths([r[:64] for r in rows], sl.LONG_CAP)
    head = kh.corridors(harness, hx, hn, table, pop_back=pop_back, seg_capacity=sl.LONG_CAP, p_max=sl.BIG_PMAX)
    later = [b for b in range(len(rows)) if got["seeds"][b].tobytes() != head["seeds"][b].tobytes()]
    assert len(later) >= 5 and all(len(rows[b]) > 64 for b in later)
    print("pop %d: n_seg %s, %d rows whose corridor changes behind point 64, stats %s" % (pop_back, got["n_seg"].tolist(), len(later), got["stats"]))
    wide = kh.corridors(harness, xyz[:4], n[:4], table, pop_back=pop_back, seg_capacity=260, p_max=sl.BIG_PMAX)
    for k in ("n_planes", "planes", "seeds", "centers"):
        assert wide[k].shape[1] == 260 and np.array_equal(wide[k][:, :sl.LONG_CAP], got[k][:4]) and not wide[k][:, sl.LONG_CAP:].any(), k
    assert np.array_equal(wide["n_seg"], got["n_seg"][:4]) and got["n_seg"][:4].min() >= 1


def test_bad_voxels_behind_point_64_cluster(harness):
    """the only voxel outside the map at index 64, 100 or len - 1 = 128, and path_len = capacity + 1: BAD_PATH with nothing, over
    the whole seg_capacity of 150; each bad row cut before its bad voxel is a good path; the good rows keep their bytes"""
    rows = sl.long_rows()
    heads = sl.bad_row_heads()
    _, table = kh.oracle_corridors(rows + heads, sl.BIG_ITR, True)
    xyz, n = ch.pack_paths(rows, sl.LONG_CAP)
    alone = kh.corridors(harness, xyz, n, table, seg_capacity=sl.LONG_CAP, p_max=sl.BIG_PMAX)
    mx, mn, good_at, bad_at = sl.mix_bad(rows, sl.LONG_CAP)
    got = kh.corridors(harness, mx, mn, table, seg_capacity=sl.LONG_CAP, p_max=sl.BIG_PMAX)
    sl.assert_bad_rows_empty(got, bad_at, kh.KEYS)
    lib.same(lib.pick(got, good_at, kh.KEYS), alone, kh.KEYS)
    assert mn[bad_at].tolist() == [150, 150, 129, sl.LONG_CAP + 1]
    hx, hn = ch.pack_paths(heads, sl.LONG_CAP)
    assert hn.tolist() == [64, 100, 128] and (kh.corridors(harness, hx, hn, table, seg_capacity=sl.LONG_CAP, p_max=sl.BIG_PMAX)["rtn"] == kh.OK).all()


@pytest.mark.parametrize("pop_back", [True, False])
def test_long_paths_cube(cube_harness, pop_back):
    """cube corridors of more than 64 polytopes (87 without pop, 81 with); at seg_capacity 70 some rows OVERFLOW with their true
    n_seg and the first 70 polytopes, others do not; bad voxels behind point 64 give BAD_PATH and zeros up to slot 159"""
    grid = ch.random_map(*sl.CUBE_MAP)
    rows = sl.cube_long_rows()
    xyz, n = ch.pack_paths(rows, sl.LONG_CAP)
    got = ch.corridors(cube_harness, grid, xyz, n, pop_back=pop_back, seg_capacity=160)
    assert (got["rtn"] == ch.OK).all() and got["n_seg"].max() == (81 if pop_back else 87)
    print("pop %d: n_seg %s" % (pop_back, got["n_seg"].tolist()))
    cut = ch.corridors(cube_harness, grid, xyz, n, pop_back=pop_back, seg_capacity=70)
    over = got["n_seg"] > 70
    assert over.any() and not over.all() and (got["n_seg"][~over] > 64).any()
    assert cut["rtn"].tolist() == [ch.OVERFLOW if o else ch.OK for o in over] and np.array_equal(cut["n_seg"], got["n_seg"])
    for k in ("n_planes", "planes", "seeds", "centers", "cube_idx"):
        assert np.array_equal(cut[k], got[k][:, :70]), k
    mx, mn, good_at, bad_at = sl.mix_bad(rows, sl.LONG_CAP)
    bad = ch.corridors(cube_harness, grid, mx, mn, pop_back=pop_back, seg_capacity=160)
    sl.assert_bad_rows_empty(bad, bad_at, CUBE_KEYS)
    lib.same(lib.pick(bad, good_at, CUBE_KEYS), got, CUBE_KEYS)
    hx, hn = ch.pack_paths(sl.bad_row_heads(), sl.LONG_CAP)
    assert (ch.corridors(cube_harness, grid, hx, hn, pop_back=pop_back, seg_capacity=160)["rtn"] == ch.OK).all()


def test_long_paths_clear(clear_harness, cube_harness):
    """radius-aware cube corridors of the same rows at floor 4 (of a field whose largest value on this map is 8): every row still
    ends OK - a cube's seed voxel is exempt from the floor - and the corridors have more than 64 polytopes, up to 142"""
    grid = ch.random_map(*sl.CUBE_MAP)
    d2 = cl.brute_d2(grid)
    xyz, n = ch.pack_paths(sl.cube_long_rows(), sl.LONG_CAP)
    got = cl.corridors(clear_harness, grid, d2, sl.CLEAR_FLOOR, xyz, n, pop_back=False, seg_capacity=160)
    assert (got["rtn"] == ch.OK).all() and got["n_seg"].max() == 142 and d2.max() == 8
    plain = ch.corridors(cube_harness, grid, xyz, n, pop_back=False, seg_capacity=160)
    assert (got["n_seg"] >= plain["n_seg"]).all() and got["cube_idx"].tobytes() != plain["cube_idx"].tobytes()


# ---- 3. batches over 1024 rows -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pool_results(harness):
    """the distinct rows of the big batches, each held against oracle.corridor_walk -> {pop_back: (table, distinct rows, result)}"""
    out = {}
    early, late, last = sl.big_pool()
    for pop_back in (True, False):
        rows = []
        for size in sl.BIG_SIZES:
            rows += sl.big_batch(size)
        uniq, _ = sl.distinct_rows(early + late + last + rows)
        want, table = kh.oracle_corridors(uniq, sl.BIG_ITR, pop_back)
        pool_table = kh.oracle_corridors(early + late + last, sl.BIG_ITR, pop_back)[1]
        assert set(pool_table) == set(table)   # a prefix asks for seeds its row asks for: the pool's table suffices
        xyz, n = ch.pack_paths(uniq, sl.BIG_CAP)
        got = kh.corridors(harness, xyz, n, table, pop_back=pop_back, seg_capacity=sl.BIG_SEG, p_max=sl.BIG_PMAX)
        kh.assert_rows_equal_oracle(got, want, uniq)
        assert got["n_seg"].max() < sl.BIG_SEG and got["n_planes"].max() <= sl.BIG_PMAX
        out[pop_back] = (table, uniq, got)
    return out


@pytest.mark.parametrize("pop_back", [True, False])
@pytest.mark.parametrize("size", sl.BIG_SIZES)
def test_big_batches(harness, pool_results, size, pop_back):
    """1025, 2048 and 2500 rows: every row holds the bytes of its distinct row (itself equal to the oracle), bad rows hold nothing;
    the stats are those of a replay of the rounds from the inputs; in that replay seeds are shared, a voxel asked for at or above
    row 1024 is owned below it, owners exist at or above row 1024 (for 2500 rows at or above 2048 too), a seed owned there is asked
    for again in a later round, and due and finished rows interleave inside a wave"""
    table, uniq, alone = pool_results[pop_back]
    rows = sl.big_batch(size)
    known, where = sl.distinct_rows(rows, uniq)
    assert len(known) == len(uniq)
    xyz, n = ch.pack_paths(rows, sl.BIG_CAP)
    got = kh.corridors(harness, xyz, n, table, pop_back=pop_back, seg_capacity=sl.BIG_SEG, p_max=sl.BIG_PMAX)
    good = where >= 0
    assert len(rows) == size and 0 < (~good).sum() < size // 8
    assert (got["rtn"][good] == kh.OK).all()
    sl.assert_bad_rows_empty(got, np.flatnonzero(~good), kh.KEYS)
    lib.same(lib.pick(got, good, kh.KEYS), lib.pick(alone, where[good], kh.KEYS), kh.KEYS)
    prop = sl.big_properties(sl.replay_rounds(rows, table, pop_back, sl.BIG_SEG), size)
    print("%d rows, pop %d: %s, pops %d" % (size, pop_back, prop, got["stats"]["pops"]))
    s = got["stats"]
    assert (s["rounds"], s["due_seeds"], s["unique_seeds"]) == (prop["rounds"], prop["due"], prop["unique"])
    assert s["unique_seeds"] < s["due_seeds"]
    assert prop["crossing"] > 0 and prop["late_owners"] > 0 and prop["interleaved"] > 0
    assert (prop["last_owners"] > 0) == (size > 2048)   # 2500 rows: the compaction's base is carried over two trips
    # a voxel that only rows from 1024 on asked for is asked for again, later, by rows behind its owner of then: the reset of the
    # owner table matters in its second trip (with 1025 rows no row lies behind row 1024)
    assert (prop["reasked"] > 0) == (size > 1025)
    assert good[1024] and xyz[1024, 0].tolist() == [5, 5, 5] and (xyz[:1024, 0] == [5, 5, 5]).all(1)[good[:1024]].any()


# ---- 4. cube inflation beyond its fixed grid -----------------------------------------------------------------------------------

def test_inflate_slots_beyond_the_fixed_grid(cube_harness):
    """4100 rows of 128 points are 524800 slots; rows 4096 .. 4099 lie wholly behind slot 524288, are walks of 128 points and end
    OVERFLOW at seg_capacity 16 with their true n_seg; the other rows end OK or BAD_PATH"""
    xyz, n, bad_at = sl.inflate_batch()
    assert xyz.shape == (sl.INFL_BATCH, sl.INFL_CAP, 3) and xyz.shape[0] * xyz.shape[1] > sl.INFL_GRID_SLOTS
    assert 4096 * sl.INFL_CAP == sl.INFL_GRID_SLOTS and (n[4096:] == 128).all() and n[:4096].max() <= 8
    got = ch.corridors(cube_harness, ch.random_map(*sl.CUBE_MAP), xyz, n, seg_capacity=sl.INFL_SEG)
    assert (got["rtn"][4096:] == ch.OVERFLOW).all() and (got["n_seg"][4096:] > sl.INFL_SEG).all()
    assert (got["n_planes"][4096:] == 6).all() and len({got["cube_idx"][b].tobytes() for b in range(4096, 4100)}) == 4
    rest = np.ones(sl.INFL_BATCH, bool)
    rest[4096:] = False
    rest[bad_at] = False
    assert (got["rtn"][rest] == ch.OK).all() and (got["rtn"][bad_at] == ch.BAD_PATH).all()
    print("rows 4096..4099: n_seg %s" % got["n_seg"][4096:].tolist())
