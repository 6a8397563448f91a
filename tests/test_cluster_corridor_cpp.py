"""The rules of direct_cluster_corridor_batch (direct_amd/csrc/cluster_corridor_math.h) on the CPU: tests/cluster_corridor_harness.py
runs the rounds - advance, unique, chunks, append, emit - over a table of polytopes from the CPU oracles, and the result is held
against oracle.corridor_walk row by row, against itself under other chunk sizes and row orders, and against planted failures.
Every row that is not planted to fail must end OK: no row is skipped or filtered."""
import functools

import numpy as np
import pytest

from tests import cluster_corridor_harness as kh
from tests import corridor_lib as lib
from tests import cube_corridor_harness as ch

CAP = kh.CAP
same = functools.partial(lib.same, keys=kh.KEYS)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return kh.build(tmp_path_factory.mktemp("cluster_corridor"))


@pytest.fixture(scope="module")
def rows():
    return kh.inside_rows()


@pytest.mark.parametrize("itr_cluster_max", [2, 50])
@pytest.mark.parametrize("pop_back", [True, False])
def test_reference_parity(harness, rows, itr_cluster_max, pop_back):
    """n_seg, n_planes, planes, seeds and centres of every row equal oracle.corridor_walk to the bit; rounds are the lock-step walk's"""
    want, table = kh.oracle_corridors(rows, itr_cluster_max, pop_back)
    xyz, n = ch.pack_paths(rows, CAP)
    got = kh.corridors(harness, xyz, n, table, pop_back=pop_back)
    assert (got["rtn"] == kh.OK).all()
    kh.assert_rows_equal_oracle(got, want, rows)
    assert all(r["rc"] == 0 for r in table.values())
    assert max(len(c) for c, _ in want) >= 4 and got["n_planes"].max() <= 16
    # every row asks for one polytope per round until it is done: the rounds are the most polytopes any row ever asked for
    assert got["stats"]["rounds"] >= got["n_seg"].max() and got["stats"]["due_seeds"] >= got["n_seg"].sum()
    assert got["stats"]["unique_seeds"] <= got["stats"]["due_seeds"]
    if itr_cluster_max == 50:
        cases = [c for c in ch.named_cases() if c["name"] != "outside_voxel"]
        u = next(i for i, c in enumerate(cases) if c["name"] == "u_turn")
        first = sum(len(c["paths"]) for c in cases[:u])
        assert got["n_seg"][first] == (1 if pop_back else 4)   # the pop path is exercised
        assert (got["stats"]["pops"] > 0) == pop_back


def test_shape_independence(harness, rows):
    """chunk sizes 1, 2 and 64 and a permuted row order give identical bytes"""
    _, table = kh.oracle_corridors(rows, 50, True)
    xyz, n = ch.pack_paths(rows, CAP)
    one = kh.corridors(harness, xyz, n, table, chunk=64)
    for chunk in (1, 2):
        got = kh.corridors(harness, xyz, n, table, chunk=chunk)
        same(got, one)
        assert got["stats"] == one["stats"]
    perm = np.random.default_rng(1).permutation(len(rows))
    p = kh.corridors(harness, xyz[perm], n[perm], table, chunk=2)
    same(p, {k: one[k][perm] for k in kh.KEYS})
    assert p["stats"] == one["stats"]
    assert (one["rtn"] == kh.OK).all()


def test_stats(harness):
    """rounds equal the rounds of the lock-step walk (the most polytopes, pops included, any row asks for); six paths from one start
    share their first seed: unique seeds < due seeds"""
    rows = kh.shared_start_rows()
    want, table = kh.oracle_corridors(rows, 50, True)
    xyz, n = ch.pack_paths(rows, CAP)
    got = kh.corridors(harness, xyz, n, table)
    assert (got["rtn"] == kh.OK).all()
    kh.assert_rows_equal_oracle(got, want, rows)
    s = got["stats"]
    assert s["unique_seeds"] < s["due_seeds"] and s["due_seeds"] >= 6
    # the lock-step walk asks once per row and round; alone, a row takes as many rounds as it asks for polytopes
    alone = [kh.corridors(harness, xyz[b:b + 1], n[b:b + 1], table)["stats"] for b in range(len(rows))]
    assert s["rounds"] == max(a["rounds"] for a in alone) and s["due_seeds"] == sum(a["due_seeds"] for a in alone)
    assert s["pops"] == sum(a["pops"] for a in alone)
    assert all(a["unique_seeds"] == a["due_seeds"] == a["rounds"] for a in alone)


@pytest.mark.parametrize("how", ["hull", "generation"])
def test_planted_failure(harness, rows, how):
    """a planted rc != 0 for one seed stops exactly the rows that ask for it, with NO_POLYTOPE and the polytopes held so far"""
    want, table = kh.oracle_corridors(rows, 50, False)
    xyz, n = ch.pack_paths(rows, CAP)
    clean = kh.corridors(harness, xyz, n, table, pop_back=False)
    # the second polytope of the longest corridor
    b0 = int(np.argmax(clean["n_seg"]))
    seed = clean["seeds"][b0, 1]
    voxel = tuple(int(v) for v in np.floor((seed - kh.LOWER) / kh.RES + 1e-9))
    assert voxel in table
    planted = dict(table)
    planted[voxel] = dict(table[voxel], rc=3) if how == "hull" else dict(table[voxel], gen_ok=0)
    got = kh.corridors(harness, xyz, n, planted, pop_back=False, chunk=2)
    hit = 0
    for b in range(len(rows)):
        at = [s for s in range(clean["n_seg"][b]) if np.array_equal(clean["seeds"][b, s], seed)]
        if not at:
            same({k: got[k][b:b + 1] for k in kh.KEYS}, {k: clean[k][b:b + 1] for k in kh.KEYS})
            continue
        hit += 1
        k = at[0]
        assert got["rtn"][b] == kh.NO_POLYTOPE and got["n_seg"][b] == k
        for key in ("n_planes", "planes", "seeds", "centers"):
            assert np.array_equal(got[key][b, :k], clean[key][b, :k]) and not got[key][b, k:].any()
    assert hit >= 1 and got["rtn"][b0] == kh.NO_POLYTOPE and got["n_seg"][b0] == 1


def test_per_row_codes(harness, rows):
    """seg_capacity one short, p_max = 8 against the 16-plane polytope, and the outside_voxel rows, each beside rows that end OK"""
    _, table = kh.oracle_corridors(rows, 50, False)
    xyz, n = ch.pack_paths(rows, CAP)
    full = kh.corridors(harness, xyz, n, table, pop_back=False)
    assert (full["rtn"] == kh.OK).all()
    need = int(full["n_seg"].max())
    cut = kh.corridors(harness, xyz, n, table, pop_back=False, seg_capacity=need - 1)
    over = full["n_seg"] >= need
    assert over.any() and not over.all()
    assert cut["rtn"].tolist() == [kh.OVERFLOW if o else kh.OK for o in over]
    assert cut["n_seg"].tolist() == [need - 1 if o else int(v) for o, v in zip(over, full["n_seg"])]
    for key in ("n_planes", "planes", "seeds", "centers"):   # without a pop the stack at that moment is the corridor's prefix
        assert np.array_equal(cut[key], full[key][:, :need - 1]), key
    # p_max = 8: a row stops at its first polytope with more than 8 planes
    assert full["n_planes"].max() == 16
    few = kh.corridors(harness, xyz, n, table, pop_back=False, p_max=8)
    stopped = 0
    for b in range(len(rows)):
        wide = [s for s in range(full["n_seg"][b]) if full["n_planes"][b, s] > 8]
        if not wide:
            assert few["rtn"][b] == kh.OK and few["n_seg"][b] == full["n_seg"][b]
            assert np.array_equal(few["planes"][b], full["planes"][b, :, :8])
            continue
        stopped += 1
        assert few["rtn"][b] == kh.TOO_MANY_PLANES and few["n_seg"][b] == wide[0]
        assert np.array_equal(few["planes"][b, :wide[0]], full["planes"][b, :wide[0], :8]) and not few["planes"][b, wide[0]:].any()
    assert 0 < stopped < len(rows)
    # the outside_voxel rows: BAD_PATH with nothing, the row between them untouched
    case = next(c for c in ch.named_cases() if c["name"] == "outside_voxel")
    bx, bn = ch.pack_paths(case["paths"], CAP)
    room = [np.asarray(case["paths"][1], np.int32)]
    _, t2 = kh.oracle_corridors(room, 50, False)
    bad = kh.corridors(harness, bx, bn, t2, pop_back=False)
    assert bad["rtn"].tolist() == case["rtn"] == [kh.BAD_PATH, kh.OK, kh.BAD_PATH, kh.BAD_PATH]
    assert bad["n_seg"][[0, 2, 3]].tolist() == [0, 0, 0] and not bad["planes"][[0, 2, 3]].any() and not bad["n_planes"][[0, 2, 3]].any()
    alone = kh.corridors(harness, bx[1:2], bn[1:2], t2, pop_back=False)
    same({k: bad[k][1:2] for k in kh.KEYS}, alone)
    # path_len 0 and path_len > path_capacity
    bn2 = bn.copy()
    bn2[0], bn2[2] = 0, CAP + 1
    assert kh.corridors(harness, bx, bn2, t2, pop_back=False)["rtn"].tolist() == [kh.BAD_PATH, kh.OK, kh.BAD_PATH, kh.BAD_PATH]


def test_float_output(harness, rows):
    """the float output is one rounding of the double output; the walk itself read the double planes (same n_seg, same codes)"""
    _, table = kh.oracle_corridors(rows, 50, True)
    xyz, n = ch.pack_paths(rows, CAP)
    d = kh.corridors(harness, xyz, n, table, dtype=np.float64)
    f = kh.corridors(harness, xyz, n, table, dtype=np.float32)
    assert (d["rtn"] == kh.OK).all()
    for key in ("n_seg", "n_planes", "rtn"):
        assert np.array_equal(d[key], f[key])
    for key in ("planes", "seeds", "centers"):
        assert f[key].dtype == np.float32 and f[key].tobytes() == d[key].astype(np.float32).tobytes(), key
