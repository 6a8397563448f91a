"""Inputs at which the strided loops of direct_amd/csrc/cluster_corridor.h and cube_corridor.h take a SECOND trip, and the property
checks that say so - TEST INFRASTRUCTURE of tests/test_corridor_strides_cpp.py (which asserts every property on the CPU harnesses)
and tests/test_gpu_corridor_strides.py (which runs the same inputs on the device).  Four families, all on the 24 x 20 x 12 map:
  wide     polytopes of more than 64 planes in the walk's plane test      (k_corr_advance, t += 64)
  long     paths of more than 64 points, corridors of more than 64 cubes  (k_corr_advance / k_cube_walk, i += 64, k += 64; k_corr_emit)
  big      batches of 1025, 2048 and 2500 rows                            (k_corr_unique, b0 += 1024 and the base_s carry)
  inflate  4100 rows of 128 points: 524800 slots                          (k_cube_inflate beyond its fixed grid of 8192 x 64)
Nothing here is computed by the device: polytopes come from the CPU oracles, corridors from the g++ harnesses."""
import numpy as np

from tests import cluster_corridor_harness as kh
from tests import cube_corridor_clear_harness as cl
from tests import cube_corridor_harness as ch

RES, LOWER, DIMS = ch.RES, ch.LOWER, ch.DIMS


def build_harness(which, tmp_path_factory, tag=""):
    """what the module-scoped harness fixtures of both stride test files return: which is "cluster", "cube" or "clear" """
    return {"cluster": kh, "cube": ch, "clear": cl}[which].build(tmp_path_factory.mktemp("corridor_strides_%s%s" % (tag, which)))

# ---- wide: more than 64 planes -------------------------------------------------------------------------------------------

WIDE_CAP, WIDE_SEG, WIDE_PMAX, WIDE_ITR = 64, 16, 96, 50
WIDE_LINE = ([7, 6, 3], [16, 14, 9])   # stacks three polytopes of more than 64 planes


def two_ball_map():
    """everything occupied but two balls of radius 5.5 voxels around (7, 10, 6) and (16, 10, 6): 1436 free voxels, whose clusters
    have curved boundaries and hulls of up to 80 planes"""
    idx = np.indices(DIMS)
    g = np.ones(DIMS, np.uint8)
    for c in ((7, 10, 6), (16, 10, 6)):
        g[sum((idx[a] - c[a]) ** 2 for a in range(3)) <= 5.5 ** 2] = 0
    return g


def out_and_back(a, b):
    return ch.line(a, b) + ch.line(b, a)[1:]


def wide_rows(seed=3, n_random=40):
    """crafted lines through both balls, out-and-back ones (so that polytopes are popped), and ch.line paths between random free voxels"""
    grid = two_ball_map()
    rows = [ch.line(*WIDE_LINE), out_and_back(*WIDE_LINE), out_and_back([7, 10, 6], [16, 10, 6]), out_and_back([4, 8, 4], [19, 12, 8]),
            ch.line([16, 14, 9], [7, 6, 3]), out_and_back([7, 14, 9], [16, 6, 3]),
            # from a seed whose polytope has more than 64 planes to a voxel that only planes of index 64 and above exclude
            ch.line([10, 6, 3], [11, 8, 9]), ch.line([13, 14, 9], [20, 12, 3])]
    free = np.argwhere(grid == 0)
    rng = np.random.default_rng(seed)
    for _ in range(n_random):
        a, b = free[rng.integers(0, len(free), 2)]
        rows.append(ch.line(a.tolist(), b.tolist()))
    assert all(len(r) <= WIDE_CAP for r in rows)
    return [np.asarray(r, np.int32).reshape(-1, 3) for r in rows]


def cut_table(table, n=64):
    """the MUTANT's table: every polytope cut to its first n planes - what a plane test that stops after one trip of 64 sees"""
    return {k: dict(t, planes=np.asarray(t["planes"])[:n]) for k, t in table.items()}


def stopped_at_first_wide(few, full, p_max):
    """few: a call with p_max below the widest polytope, full: the same call (no pop, every row OK) with room for all.  A row with a
    polytope of more than p_max planes ends TOO_MANY_PLANES at the first such, holding the head of its full corridor; the others
    end OK with all of it.  -> the number of stopped rows"""
    stopped = 0
    for b in range(len(full["n_seg"])):
        wide = [s for s in range(full["n_seg"][b]) if full["n_planes"][b, s] > p_max]
        k = wide[0] if wide else int(full["n_seg"][b])
        assert few["rtn"][b] == (kh.TOO_MANY_PLANES if wide else kh.OK) and few["n_seg"][b] == k, (b, few["rtn"][b], few["n_seg"][b], k)
        assert np.array_equal(few["planes"][b, :k], full["planes"][b, :k, :p_max]) and not few["planes"][b, k:].any(), b
        for key in ("n_planes", "seeds", "centers"):
            assert np.array_equal(few[key][b, :k], full[key][b, :k]) and not few[key][b, k:].any(), (b, key)
        stopped += bool(wide)
    return stopped


# ---- long: more than 64 points -------------------------------------------------------------------------------------------

LONG_CAP = 150                                   # no multiple of 64
LONG_LENGTHS = (64, 65, 128, 129, 150, 150, 20, 100, 63, 129, 3, 150, 77, 128)
CUBE_MAP = (80, 0.15)                            # ch.random_map(*CUBE_MAP): the cube corridors' map
CLEAR_FLOOR = 4                                  # min_d2 of the radius-aware case; the field of that map reaches 8


def long_rows():
    """14 random walks whose lengths sit on and around the wave's 64 and 128, up to the path capacity of 150"""
    grid = np.zeros(DIMS, np.uint8)
    return [ch.random_paths(grid, 1, seed=100 + j, length=n)[0] for j, n in enumerate(LONG_LENGTHS)]


def cube_long_rows():
    """the 16 walks of 150 points whose cube corridors have up to 87 polytopes, then long_rows()"""
    return ch.random_paths(np.zeros(DIMS, np.uint8), 16, seed=5, length=LONG_CAP) + long_rows()


def bad_long_rows(rows):
    """four BAD_PATH rows made from `rows` (long_rows() order): the only voxel outside the map at index 64, at index 100 and at index
    len - 1 of a path of 129 points; the fourth is a good path whose path_len the caller sets to the capacity + 1.
    -> (rows, index of the row whose length is to be overwritten)"""
    a, b, c = rows[4].copy(), rows[5].copy(), rows[3].copy()
    assert len(a) == 150 and len(b) == 150 and len(c) == 129
    a[64] = [DIMS[0], a[64][1], a[64][2]]
    b[100] = [b[100][0], -1, b[100][2]]
    c[128] = [c[128][0], c[128][1], DIMS[2]]
    for p in (a, b, c):
        assert ((p < 0) | (p >= np.array(DIMS))).any(1).sum() == 1
    return [a, b, c, rows[11].copy()], 3


def bad_row_heads():
    """the three bad rows cut just before their bad voxel: valid paths of 64, 100 and 128 points"""
    bad, _ = bad_long_rows(long_rows())
    return [bad[0][:64], bad[1][:100], bad[2][:128]]


def mix_bad(good, cap):
    """good rows with the four bad rows between them -> (xyz, n, indices of the good rows, indices of the bad rows)"""
    bad, over = bad_long_rows(long_rows())
    bad_at = [1, 5, len(good) // 2 + 2, len(good) + 2]   # ascending, so that an insertion moves no earlier one
    rows = list(good)
    for i, r in zip(bad_at, bad):
        rows.insert(i, r)
    good_at = [i for i in range(len(rows)) if i not in bad_at]
    xyz, n = ch.pack_paths(rows, cap)
    n[bad_at[over]] = cap + 1
    assert all(rows[i] is r for i, r in zip(bad_at, bad)) and len(good_at) == len(good)
    return xyz, n, good_at, bad_at


def assert_bad_rows_empty(got, bad_at, keys):
    """BAD_PATH, n_seg 0 and zeros across the whole seg_capacity"""
    for b in bad_at:
        assert got["rtn"][b] == ch.BAD_PATH and got["n_seg"][b] == 0, (b, got["rtn"][b], got["n_seg"][b])
        for k in keys:
            if k not in ("rtn", "n_seg"):
                assert not got[k][b].any(), (b, k)


# ---- big: more than 1024 rows ---------------------------------------------------------------------------------------------

BIG_CAP, BIG_SEG, BIG_PMAX, BIG_ITR = 40, 16, 20, 50   # the longest corridor of the pool has 15 polytopes, the widest polytope 16 planes
BIG_SIZES = (1025, 2048, 2500)
ECHO_SEED = [20, 6, 5]   # the seed of late[0]'s third polytope, which no early row asks for


def big_pool():
    """-> (early, late, last): the distinct base rows of the big batches on ch.crafted_map(), none longer than 40 points.  `late`
    rows are placed at row 1024 and above ONLY, `last` rows at row 2048 and above only: they share their start [5, 5, 5] with rows
    of `early` (so that in the first round their owner lies below row 1024) and later ask for seeds no row before them asks for
    (so that they own them, in the second and in the third trip of the compaction).  The last of `late` is an ECHO of late[0]: it
    asks for late[0]'s third seed one round after late[0] did.  With late[0] at row 1024 and the echo behind it, an owner entry
    that the round before failed to reset would outrank every row that asks now."""
    shared = kh.shared_start_rows()
    ends = ([20, 9, 9], [12, 2, 10], [15, 18, 2], [22, 1, 1], [10, 17, 6], [18, 5, 0])
    tail = [np.asarray(ch.line([5, 5, 5], [8, 5, 5]) + ch.line([9, 5, 5], e), np.int32) for e in ends]   # out of the room's door, then away
    early = kh.inside_rows() + shared + [p[:BIG_CAP] for p in long_rows()]
    at = next(i for i, v in enumerate(tail[0]) if v.tolist() == ECHO_SEED)
    echo = np.asarray([[5, 5, 5], [13, 4, 4], [12, 12, 5]] + tail[0][at:].tolist(), np.int32)   # the room, the enclosed voxel, the tunnel
    return [np.asarray(p, np.int32).reshape(-1, 3) for p in early], tail[:4] + [echo], tail[4:]


def big_batch(size, seed=11):
    """-> list of rows: base rows, prefixes of them (a prefix asks for seeds its row asks for) and BAD_PATH rows, drawn with a fixed
    seed; late rows only from row 1024 on, one of them AT row 1024, last rows only from row 2048 on"""
    early, late, last = big_pool()
    rng = np.random.default_rng(seed + size)
    rows = []
    for b in range(size):
        u = rng.random()
        p = early[rng.integers(0, len(early))]
        if u < 0.08:
            rows.append(np.asarray([[0, DIMS[1], 0]], np.int32) if u < 0.04 else np.zeros((0, 3), np.int32))   # outside / empty
        elif u < 0.35:
            rows.append(p[:rng.integers(1, len(p) + 1)])
        elif u < 0.5 and b >= 1024:
            rows.append(late[rng.integers(0, len(late))])
        elif u < 0.6 and b >= 2048:
            rows.append(last[rng.integers(0, len(last))])
        else:
            rows.append(p)
    rows[1024] = late[0]
    if size > 1025:
        rows[1030] = late[-1]
    if size > 2048:
        rows[2048] = last[0]
    return rows


def ask_sequence(row, table, pop_back, seg_capacity):
    """the voxels a row asks polytopes for, in order - its k-th ask falls into round k, whatever the other rows do.  The walk of
    cluster_corridor_math.h::advance restated on the oracle table; a row that is not a valid path asks for nothing."""
    row = np.asarray(row, np.int64).reshape(-1, 3)
    if len(row) == 0 or (row < 0).any() or (row >= np.array(DIMS)).any():
        return []

    def outside(c, planes):
        q = np.asarray(planes, np.float64).reshape(-1, 4)
        return bool((q[:, 0] * c[0] + q[:, 1] * c[1] + q[:, 2] * c[2] + q[:, 3] > 0.01).any())

    stack, asks, lst = [], [], None
    for v in row:
        cur = v * RES + 0.5 * RES + LOWER
        if lst is not None and (cur == lst).all():
            continue
        if pop_back and len(stack) > 1 and not outside(cur, stack[-2]):
            stack.pop()
        if not stack or outside(cur, stack[-1]):
            if len(stack) >= seg_capacity:
                break
            key = tuple(int(i) for i in v)
            asks.append(key)
            if table[key]["rc"] != 0:
                break
            stack.append(table[key]["planes"])
        lst = cur
    return asks


def replay_rounds(rows, table, pop_back, seg_capacity):
    """-> list over rounds of dict(due: bool [B], owner: {voxel: smallest due row}, asks: per row its voxel or None); identical rows
    share one ask sequence"""
    memo, asks = {}, []
    for r in rows:
        key = np.asarray(r, np.int32).tobytes()
        if key not in memo:
            memo[key] = ask_sequence(r, table, pop_back, seg_capacity)
        asks.append(memo[key])
    rounds = []
    for k in range(max(len(a) for a in asks)):
        due = np.array([len(a) > k for a in asks])
        owner = {}
        for b in np.flatnonzero(due):
            owner.setdefault(asks[b][k], int(b))
        rounds.append(dict(due=due, owner=owner, asks=[a[k] if len(a) > k else None for a in asks]))
    return rounds


def big_properties(rounds, size):
    """what makes a batch exercise the second and third trip of k_corr_unique's loops -> dict(rounds, due, unique: the stats the
    call must report; crossing: asks from row 1024 on whose owner lies below it; late_owners / last_owners: owners from row 1024 /
    2048 on; reasked: owners that a table entry left behind by an earlier round's owner from row 1024 on would outrank;
    interleaved: waves in which a row that is not due lies between two due ones), each summed over the rounds"""
    due = sum(int(r["due"].sum()) for r in rounds)
    unique = sum(len(r["owner"]) for r in rounds)
    crossing = late_owners = last_owners = interleaved = reasked = 0
    left = {}   # voxel -> its owner in the latest earlier round in which only rows from 1024 on asked for it
    for r in rounds:
        reasked += sum(v in left and left[v] < o for v, o in r["owner"].items())   # a stale entry would outrank this round's owner
        for v, o in r["owner"].items():
            left.pop(v, None)
            if o >= 1024:
                left[v] = o
        for b in np.flatnonzero(r["due"][1024:]) + 1024:
            crossing += r["owner"][r["asks"][b]] < 1024     # asked at or above row 1024, owned below it
        late_owners += sum(o >= 1024 for o in r["owner"].values())
        last_owners += sum(o >= 2048 for o in r["owner"].values())
        d = r["due"]
        for w in range(0, size, 64):
            lanes = np.flatnonzero(d[w:w + 64])
            interleaved += len(lanes) >= 2 and (lanes[-1] - lanes[0] + 1) > len(lanes)   # a finished row between two due ones
    return dict(rounds=len(rounds), due=due, unique=unique, crossing=int(crossing), late_owners=int(late_owners),
                last_owners=int(last_owners), reasked=int(reasked), interleaved=int(interleaved))


# ---- inflate: more than 524288 slots ---------------------------------------------------------------------------------------

INFL_BATCH, INFL_CAP, INFL_SEG = 4100, 128, 16
INFL_GRID_SLOTS = 8192 * 64    # the slots k_cube_inflate's fixed grid covers in its first trip


def inflate_batch():
    """-> (xyz, n, bad rows): rows 4096 .. 4099 are walks of 128 points - wholly beyond the first trip -, all others paths of at most
    8 points cycled from kh.inside_rows(), a few of them BAD_PATH"""
    short = [np.asarray(p, np.int32).reshape(-1, 3)[:8] for p in kh.inside_rows()]
    rows = [short[b % len(short)] for b in range(INFL_BATCH)]
    bad_at = [7, 1000, 4000]
    for b in bad_at:
        rows[b] = np.asarray([[3, 3, 3], [DIMS[0], 3, 3]], np.int32)
    walks = [p for p in long_rows() if len(p) == 128] + [p[:128] for p in long_rows() if len(p) == 150]
    rows[4096:4100] = walks[:4]
    xyz, n = ch.pack_paths(rows, INFL_CAP)
    assert (n[4096:] == 128).all()
    return xyz, n, bad_at


def distinct_rows(rows, known=()):
    """-> (the distinct valid rows: `known`, then the others in order of first appearance; per row its index among them, or -1 for
    a row that is no valid path)"""
    uniq = [np.ascontiguousarray(r, np.int32).reshape(-1, 3) for r in known]
    seen = {r.tobytes(): i for i, r in enumerate(uniq)}
    where = []
    for r in rows:
        r = np.ascontiguousarray(r, np.int32).reshape(-1, 3)
        if len(r) == 0 or (r < 0).any() or (r >= np.array(DIMS)).any():
            where.append(-1)
            continue
        if r.tobytes() not in seen:
            seen[r.tobytes()] = len(uniq)
            uniq.append(r)
        where.append(seen[r.tobytes()])
    return uniq, np.array(where)
