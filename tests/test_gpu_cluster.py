"""Corridor-cluster kernels (include/direct_cluster.h) against the reference: bit-exact integer / byte parity.

k_convex + k_resolve are checked against the REFERENCE'S OWN serialConvexTest (oracle/_ref, built from its source)
on the committed golden vectors and on fresh scenes; the whole polygonGeneration against the restated loops with
the reference function plugged in.  PARITY PINNED."""
import os

import numpy as np
import pytest

from direct_amd import cluster, problems
from oracle import clusterapi as ca
from tests import cluster_shell_lib as csl

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", ["a", "b"])
def test_convex_test_kernel_matches_reference_golden(built, name):
    g = np.load(os.path.join(GOLD, "cluster_convex_%s.npz" % name))
    gen = cluster.ClusterGenerator(g["grid"].shape, max_batch=1, cluster_capacity=4096, candidate_capacity=1024)
    gen.set_map(g["grid"])
    clu, cc, acc = gen.convex_test(g["inside"], g["cand"], g["cluster"])
    assert np.array_equal(clu, g["can_clu"])
    assert np.array_equal(cc, g["can_can"])        # the whole packed triangle, every ray
    assert np.array_equal(acc, g["accept"])
    gen.close()


def test_polygon_generation_matches_golden(built):
    g = np.load(os.path.join(GOLD, "cluster_polygon_48.npz"))
    gen = cluster.ClusterGenerator(g["grid"].shape, max_batch=16, cluster_capacity=8192, candidate_capacity=4096)
    gen.set_map(g["grid"])
    r = gen.polygon_generation(g["seeds"])
    assert (r["rtn"] == 0).all()
    assert np.array_equal(r["vertex_idx"], g["vertex_idx"])
    assert np.array_equal(r["cluster_num"], g["cluster_num"]) and np.array_equal(r["iters"], g["iters"])
    assert np.array_equal(np.concatenate(r["clusters"]), g["cluster_xyz"])   # same voxels in the same order
    # a second call on the same handle (flagClear) and a different batch composition give the same rows
    r2 = gen.polygon_generation(g["seeds"][::-1][:5])
    for q in range(5):
        assert np.array_equal(r2["clusters"][q], r["clusters"][len(g["seeds"]) - 1 - q])
    gen.close()


def test_large_candidate_capacity_takes_the_general_kernels(built):
    """Above 16384 candidates per round the row of the bit matrix no longer fits the registers / LDS of the fast
    accept loop and of k_convex's queued candidate rays: the general kernels (k_resolve_pipe, un-queued rows) run
    instead and must give the same clusters."""
    g = np.load(os.path.join(GOLD, "cluster_polygon_48.npz"))
    gen = cluster.ClusterGenerator(g["grid"].shape, max_batch=16, cluster_capacity=8192, candidate_capacity=20000)
    gen.set_map(g["grid"])
    r = gen.polygon_generation(g["seeds"])
    assert (r["rtn"] == 0).all()
    assert np.array_equal(r["cluster_num"], g["cluster_num"]) and np.array_equal(r["iters"], g["iters"])
    assert np.array_equal(np.concatenate(r["clusters"]), g["cluster_xyz"])
    gen.close()


def test_polygon_generation_on_a_larger_map_against_the_oracle(built):
    """120 x 120 x 24 map, 48 seeds in one batch, against the oracle with the reference's serialConvexTest."""
    grid, seeds = problems.make_voxel_map()
    seeds = seeds[:48]
    gen = cluster.ClusterGenerator(grid.shape, max_batch=48, cluster_capacity=50000, candidate_capacity=10000)
    gen.set_map(grid)
    r = gen.polygon_generation(seeds, itr_inflate_max=1000, itr_cluster_max=50)
    have_ref = ca.ref_lib() is not None
    ca.use_reference_convex_test(have_ref)
    try:
        for b in range(0, 48, 4):
            v, cl, it, rc = ca.polygon_generation(grid, seeds[b])
            assert rc == 0 and r["rtn"][b] == 0
            assert np.array_equal(r["vertex_idx"][b], v) and r["iters"][b] == it
            assert np.array_equal(r["clusters"][b], cl)
    finally:
        ca.use_reference_convex_test(False)
    # size-independent properties of every row: free voxels only, no duplicates, cube obstacle free
    for b in range(48):
        cl, v = r["clusters"][b], r["vertex_idx"][b]
        assert not grid[cl[:, 0], cl[:, 1], cl[:, 2]].any()
        assert len(np.unique(cl, axis=0)) == len(cl)
        assert not grid[v[7]:v[1] + 1, v[15]:v[9] + 1, v[23]:v[17] + 1].any()
    # cluster-off mode of paramSet (1000, 0): the cluster is the cube's surface
    r0 = gen.polygon_generation(seeds[:4], 1000, 0)
    for b in range(4):
        assert np.array_equal(r0["clusters"][b], ca.polygon_generation(grid, seeds[b], 1000, 0)[1]) and r0["iters"][b] == 0
    assert gen.last_ms() > 0
    gen.close()


def test_edge_cases(built):
    grid = np.zeros((12, 10, 6), np.uint8)
    grid[5, :, :] = 1                      # a wall splits the map
    grid[0, 0, 0] = 1
    gen = cluster.ClusterGenerator(grid.shape, max_batch=8, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
    seeds = np.array([[2, 3, 3], [20, 0, 0], [-1, 2, 2], [8, 4, 2]], np.int32)
    r = gen.polygon_generation(seeds)
    assert r["rtn"][1] == cluster.CLUSTER_BAD_SEED and r["rtn"][2] == cluster.CLUSTER_BAD_SEED
    assert r["cluster_num"][1] == 0 and r["cluster_num"][2] == 0
    assert r["rtn"][0] == cluster.CLUSTER_OVERFLOW     # the 5 x 10 x 6 half-room has more than 64 surface voxels
    gen.close()
    gen = cluster.ClusterGenerator(grid.shape, max_batch=8, cluster_capacity=4096, candidate_capacity=1024)
    gen.set_map(grid)
    r = gen.polygon_generation(seeds[[0, 3]])
    for b, s in enumerate(seeds[[0, 3]]):
        v, cl, it, rc = ca.polygon_generation(grid, s)
        assert np.array_equal(r["clusters"][b], cl) and np.array_equal(r["vertex_idx"][b], v) and r["iters"][b] == it
    # degenerate cube (one voxel thick): no clustering (cluster_server_cpu.cpp:509-518)
    thin = np.ones((6, 6, 6), np.uint8)
    thin[2, 1:5, 1:5] = 0
    g2 = cluster.ClusterGenerator(thin.shape, max_batch=1, cluster_capacity=256, candidate_capacity=256)
    g2.set_map(thin)
    rt = g2.polygon_generation([[2, 2, 2]])
    v, cl, it, rc = ca.polygon_generation(thin, (2, 2, 2))
    assert np.array_equal(rt["clusters"][0], cl) and rt["iters"][0] == 0 and len(cl) == 16
    # a seed enclosed on all sides: the one-voxel cube
    one = np.ones((5, 5, 5), np.uint8)
    one[2, 2, 2] = 0
    g3 = cluster.ClusterGenerator(one.shape, max_batch=1, cluster_capacity=16, candidate_capacity=16)
    g3.set_map(one)
    ro = g3.polygon_generation([[2, 2, 2]])
    assert ro["cluster_num"][0] == 1 and np.array_equal(ro["clusters"][0], [[2, 2, 2]])
    g2.close(); g3.close(); gen.close()


# ---- the code paths picked by candidate count and cluster size (tests/cluster_shell_lib.py) ------------------------------
# k_resolve_fast keeps 1 / 2 / 4 row words per lane for candidates below 4096 / 8192 / 16384, k_resolve_pipe and k_convex's
# un-queued rows take over above a candidate CAPACITY of 16384, convex_one treats cluster chunks from the 256th on apart; the
# fixtures above stay below 1336 candidates per round (the 48-seed golden) and 3126 (the big map's first round).  The scenes'
# answers are in tests/golden/cluster_shell_classes.npz (the oracle with the reference's serialConvexTest; regenerated on the
# CPU by tests/test_cluster_shell_scenes.py); nothing below runs the oracle on more than a few thousand rays.
_SHELL = {}


def _shell_gold():
    if not _SHELL:
        _SHELL.update(np.load(os.path.join(GOLD, "cluster_shell_classes.npz")))
    return _SHELL


def _shell_gen(sc, candidate_capacity, cluster_capacity=None, max_batch=1, grid=None):
    g = _shell_gold()
    ccap = int(g[sc["name"] + "_sizes"][-1]) + 1024 if cluster_capacity is None else cluster_capacity
    gen = cluster.ClusterGenerator(sc["grid"].shape, max_batch=max_batch, cluster_capacity=ccap, candidate_capacity=candidate_capacity)
    gen.set_map(sc["grid"] if grid is None else grid)
    return gen


def _assert_row_is_fixture(r, b, name, rounds=csl.ROUNDS):
    g = _shell_gold()
    n = int(g[name + "_sizes"][rounds])
    why = csl.explain(name, g, r["clusters"][b])
    assert r["rtn"][b] == cluster.CLUSTER_OK, why
    assert np.array_equal(r["vertex_idx"][b], g[name + "_vertex_idx"]), why
    assert r["iters"][b] == rounds and r["cluster_num"][b] == n, why
    assert np.array_equal(r["clusters"][b], g[name + "_cluster"][:n]), why        # same voxels in the same order


def _assert_same_rows(r, b, q, c):
    assert r["rtn"][b] == q["rtn"][c] and r["iters"][b] == q["iters"][c] and r["cluster_num"][b] == q["cluster_num"][c]
    assert np.array_equal(r["vertex_idx"][b], q["vertex_idx"][c]) and np.array_equal(r["clusters"][b], q["clusters"][c])


# n16384: its second round has more than 16384 candidates, more than the fast path can hold; one round = the fixture's first prefix
@pytest.mark.parametrize("name,rounds", [("s28", 2), ("s38", 2), ("n4095", 2), ("n4096", 2), ("n4097", 2), ("n8192", 2),
                                         ("n8193", 2), ("n16384", 1)])
def test_fast_accept_loop_in_every_candidate_range(built, name, rounds):
    """k_resolve_fast with real candidates in its 1-, 2- and 4-word ranges, and exactly at / next to 4096, 8192 and 16384."""
    sc = csl.scene(name)
    gen = _shell_gen(sc, 16384)
    r = gen.polygon_generation([sc["seed"]], itr_cluster_max=rounds)
    _assert_row_is_fixture(r, 0, name, rounds)
    _assert_same_rows(gen.polygon_generation([sc["seed"]], itr_cluster_max=rounds), 0, r, 0)   # a second call on the same handle
    gen.close()


@pytest.mark.parametrize("name", ["s54", "n16384", "n16385"])
def test_general_kernels_with_more_than_16384_candidates(built, name):
    """candidate_capacity 24576 = 384 row words: k_resolve_pipe past its four register words, k_convex's un-queued rows."""
    sc = csl.scene(name)
    assert _shell_gold()[name + "_n_cand"].max() > 16384
    gen = _shell_gen(sc, 24576)
    r = gen.polygon_generation([sc["seed"]], itr_cluster_max=csl.ROUNDS)
    _assert_row_is_fixture(r, 0, name)
    gen.close()


def test_fast_and_general_kernels_agree(built):
    sc = csl.scene("s38")
    out = []
    for kcap in (16384, 24576):
        gen = _shell_gen(sc, kcap)
        out.append(gen.polygon_generation([sc["seed"]], itr_cluster_max=csl.ROUNDS))
        gen.close()
    _assert_row_is_fixture(out[0], 0, "s38")
    _assert_row_is_fixture(out[1], 0, "s38")
    _assert_same_rows(out[0], 0, out[1], 0)


def test_mixed_batch_around_a_large_round(built):
    sc = csl.scene("s28")
    grid, pocket, room = csl.with_side_rooms(sc)
    gen = _shell_gen(sc, 16384, max_batch=4, grid=grid)
    seeds = np.array([sc["seed"], pocket, [sc["grid"].shape[0], 3, 3], sc["seed"]], np.int32)
    r = gen.polygon_generation(seeds, itr_cluster_max=csl.ROUNDS)
    single = gen.polygon_generation(seeds[:1], itr_cluster_max=csl.ROUNDS)
    for b in (0, 3):
        _assert_row_is_fixture(r, b, "s28")
        _assert_same_rows(r, b, single, 0)
    assert r["rtn"][2] == cluster.CLUSTER_BAD_SEED and r["cluster_num"][2] == 0
    v, cl, it, rc = ca.polygon_generation(grid, pocket, itr_cluster_max=csl.ROUNDS)
    assert len(cl) == 1 and r["rtn"][1] == cluster.CLUSTER_OK and r["iters"][1] == it == 0
    assert np.array_equal(r["clusters"][1], cl) and np.array_equal(r["vertex_idx"][1], v)
    gen.close()


@pytest.mark.parametrize("site,name,kcap,ccap,rounds", [
    ("cluster capacity in k_resolve_fast", "s28", 16384, 6000, 2),
    ("cluster capacity in k_resolve_pipe", "s28", 24576, 6000, 2),
    ("candidate capacity in k_compact_write", "s28", 4096, 16384, 2),
    ("candidate capacity by one, second round", "n16384", 16384, 50000, 2),
    ("candidate capacity by one, first round", "n16385", 16384, 50000, 2)])
def test_overflow_inside_a_round(built, site, name, kcap, ccap, rounds):
    """A row that overflows in the middle of a round reports CLUSTER_OVERFLOW and a VALID PREFIX of its cluster (how long a
    prefix is the kernel's business: the fast loop keeps the rounds before, the general one fills the capacity); the row next
    to it in the batch is what it is alone."""
    g = _shell_gold()
    sc = csl.scene(name)
    grid, pocket, room = csl.with_side_rooms(sc)
    surface, after_first = int(g[name + "_sizes"][0]), int(g[name + "_sizes"][1])
    if site.startswith("cluster capacity"):
        assert surface < ccap < after_first                         # the first round's accepted candidates do not fit
    elif name == "s28":
        assert g[name + "_n_cand"][0] > kcap and ccap > g[name + "_sizes"][-1]
    else:
        rnd = 1 if name == "n16384" else 0                          # n16384's first round fills the capacity to the last slot
        assert g[name + "_n_cand"][rnd] > kcap and (g[name + "_n_cand"][:rnd] <= kcap).all() and ccap > g[name + "_sizes"][-1]
        assert g[name + "_n_cand"][0] == kcap + (name == "n16385")
    gen = _shell_gen(sc, kcap, cluster_capacity=ccap, max_batch=2, grid=grid)
    for seeds in (np.array([sc["seed"], room], np.int32), np.array([room, sc["seed"]], np.int32)):
        b = 0 if (seeds[0] == sc["seed"]).all() else 1
        r = gen.polygon_generation(seeds, itr_cluster_max=rounds)
        n = int(r["cluster_num"][b])
        why = "%s: cluster_num %d\n%s" % (site, n, csl.explain(name, g, r["clusters"][b]))
        assert r["rtn"][b] == cluster.CLUSTER_OVERFLOW, why
        assert surface <= n <= ccap, why
        assert np.array_equal(r["clusters"][b], g[name + "_cluster"][:n]), why
        assert np.array_equal(r["vertex_idx"][b], g[name + "_vertex_idx"]), why
        # the neighbour: the 3 x 3 x 3 room whose x wall is open but for its stopper, against the oracle and against the row alone
        v, cl, it, rc = ca.polygon_generation(grid, room, itr_cluster_max=rounds)
        assert rc == 0 and it >= 1 and len(cl) > 26
        assert r["rtn"][1 - b] == cluster.CLUSTER_OK and r["iters"][1 - b] == it
        assert np.array_equal(r["clusters"][1 - b], cl) and np.array_equal(r["vertex_idx"][1 - b], v)
        _assert_same_rows(gen.polygon_generation([room], itr_cluster_max=rounds), 0, r, 1 - b)
    gen.close()


def test_convex_test_with_more_than_256_cluster_chunks(built):
    """68000 cluster voxels = 266 chunks of 256: convex_one's chunks from the 256th on have no entry in its skip table."""
    c = csl.chunk_scene()
    gen = cluster.ClusterGenerator(c["grid"].shape, max_batch=1, cluster_capacity=70000, candidate_capacity=64)
    gen.set_map(c["grid"])
    clu, cc, acc = gen.convex_test(c["inside"], c["cand"], c["cluster"])
    gen.close()
    R, name = (ca.ref_lib(), "ref_serial_convex_test") if ca.ref_lib() is not None else (ca.lib(), "cl_serial_convex_test")
    want = ca.serial_convex_test(R, name, c["cand"], c["cluster"], c["inside"], c["grid"], c["grid"].shape)
    assert min(int(want.sum()), int((want == 0).sum())) >= 8
    assert np.array_equal(clu, want), np.flatnonzero(clu != want)
    assert np.array_equal(acc, ca.accept_sequential(clu, cc))


def test_convex_test_rows_wider_than_64_words(built):
    """The first round of the s28 scene (5154 candidates: rows of up to 81 words) at the kernel level, through the queued rows
    (capacity 16384) and the un-queued ones (24576)."""
    g = _shell_gold()
    sc = csl.scene("s28")
    v, surf, inside, cand = csl.first_round_state(sc)
    n = len(cand)
    assert n == g["s28_n_cand"][0] and n > 4096 + 500
    out = []
    for kcap in (16384, 24576):
        gen = cluster.ClusterGenerator(sc["grid"].shape, max_batch=1, cluster_capacity=8192, candidate_capacity=kcap)
        gen.set_map(sc["grid"])
        out.append(gen.convex_test(inside, cand, surf))
        gen.close()
    (clu, cc, acc), (clu2, cc2, acc2) = out
    assert np.array_equal(clu, clu2) and np.array_equal(cc, cc2) and np.array_equal(acc, acc2)
    assert np.array_equal(acc, ca.accept_sequential(clu, cc))
    # against the fixture: the first round's per-range counts, and the accepted candidates are the cluster's next voxels
    for q in g["s28_report"]:
        if q[0] == 0:
            assert int(clu[q[1]:q[2]].sum()) == q[3] and int(acc[q[1]:q[2]].sum()) == q[4], (q, csl.explain("s28", g, surf))
    assert np.array_equal(cand[acc == 1], g["s28_cluster"][g["s28_sizes"][0]:g["s28_sizes"][1]])
    R, name = (ca.ref_lib(), "ref_serial_convex_test") if ca.ref_lib() is not None else (ca.lib(), "cl_serial_convex_test")
    rng = np.random.default_rng(5)
    i = np.concatenate([rng.integers(1, n, 1400), rng.integers(4096, n, 600)])
    j = (rng.random(2000) * i).astype(np.int64)
    assert (i >= 4096).sum() >= 500 and (j < i).all() and (j >= 4096).sum() >= 20
    blocked = 0
    for a, b in zip(i, j):
        want = ca.serial_convex_test(R, name, cand[a:a + 1], cand[b:b + 1], inside, sc["grid"], sc["grid"].shape)[0]
        assert cc[a * (a - 1) // 2 + b] == want, (a, b)
        blocked += want == 0
    # a uniform sample holds few blocked pairs: every blocked pair of a row past 4096 as well (they decide the chain)
    rows = np.flatnonzero((clu == 1) & (acc == 0))
    rows = rows[rows >= 4096][:40]
    assert len(rows) >= 3
    for a in rows:
        for b in np.flatnonzero(cc[a * (a - 1) // 2:a * (a - 1) // 2 + a] == 0):
            assert ca.serial_convex_test(R, name, cand[a:a + 1], cand[b:b + 1], inside, sc["grid"], sc["grid"].shape)[0] == 0, (a, b)
            blocked += 1
    assert blocked >= 3


def test_random_scenes_on_the_device(built):
    """The twelve random scenes whose answers the reference gave (tests/golden/make_cluster_golden.py), asked of k_convex."""
    g = np.load(os.path.join(GOLD, "cluster_convex_random_12.npz"))
    for trial in range(int(g["n"])):
        grid, inside, cand, clu, want = (g["%s_%d" % (k, trial)] for k in ("grid", "inside", "cand", "cluster", "can_clu"))
        gen = cluster.ClusterGenerator(grid.shape, max_batch=1, cluster_capacity=64, candidate_capacity=64)
        gen.set_map(grid)
        got, cc, acc = gen.convex_test(inside, cand, clu)
        gen.close()
        assert np.array_equal(got, want), (trial, np.flatnonzero(got != want))
        assert np.array_equal(acc, ca.accept_sequential(got, cc))
