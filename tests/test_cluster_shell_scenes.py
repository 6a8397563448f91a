"""The inputs of the cluster kernels' large-round tests (tests/cluster_shell_lib.py, tests/golden/cluster_shell_classes.npz) on
the CPU: the generator gives the boxes and the exact candidate counts it promises, the oracle regenerates the committed
fixture, and every scene meets the CONDITIONS ON THE INPUTS - per candidate-index range [0, 4096), [4096, 8192),
[8192, 16384), [16384, n), in the first round that reaches it: at least 100 accepted candidates, at least 3 that see the old
cluster and are rejected by the chain, at least 3 that fail the cluster test, and in the first round's highest range at least 3 chain
rejections that only accepted candidates OF that range decide - the ones that need the range's own words of the accepted
bitset; every range above the first has such a scene (cluster_shell_lib.unmet_conditions; a tail of fewer than 512 candidates only has to hold an accepted one).  With the restatement alone, and with the reference's own
serialConvexTest plugged in where oracle/_ref is built.

Measured on the CPU (8 cores, four scenes at a time): the ten scenes take about two minutes through the restatement and as long again
through the reference's function; one scene alone 2.5 s (n4095 ... n4097), 5 s (s28), 13 - 20 s (n8192, n8193, s38) and 60 s
(n16384, n16385, s54).  The time is candidates x cluster rays of two rounds - the accepted candidates, which are most, meet no
early exit."""
import os

import numpy as np
import pytest

from oracle import clusterapi as ca
from tests import cluster_shell_lib as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_shell_classes.npz")
_RUNS = {}


def _runs(reference):
    if reference not in _RUNS:
        _RUNS[reference] = L.run_scenes(L.scene_names(), reference=reference)
    return _RUNS[reference]


@pytest.mark.parametrize("name", L.scene_names())
def test_generator_gives_the_box_and_the_candidate_count(name):
    sc = L.scene(name)
    assert len(set(sc["cube"])) == 3 and len(set(sc["grid"].shape)) == 3          # a stride mix-up cannot hide
    v, surf, inside, cand = L.first_round_state(sc)
    x0, x1, y0, y1, z0, z1 = sc["box"]
    assert (v[7], v[1], v[15], v[9], v[23], v[17]) == (x0, x1, y0, y1, z0, z1)
    assert (x1 - x0 + 1, y1 - y0 + 1, z1 - z0 + 1) == sc["cube"] and len(surf) == sc["surface"]
    # every obstacle of the first shell removes exactly one candidate
    shell = np.zeros(sc["grid"].shape, bool)
    shell[x0 - 1:x1 + 2, y0 - 1:y1 + 2, z0 - 1:z1 + 2] = True
    shell[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = False
    assert len(cand) == int(shell.sum()) - int(sc["grid"][shell].sum()) == sc["expect_candidates"]
    if name.startswith("n"):
        assert len(cand) == int(name[1:])
    assert shell[cand[:, 0], cand[:, 1], cand[:, 2]].all() and len(np.unique(cand, axis=0)) == len(cand)


def test_the_scenes_reach_every_class():
    n = {name: L.scene(name)["expect_candidates"] for name in L.scene_names()}
    assert 4096 < n["s28"] < 8192 < n["s38"] < 16384 < n["s54"] < 24576
    assert sorted(v for k, v in n.items() if k.startswith("n")) == [4095, 4096, 4097, 8192, 8193, 16384, 16385]


@pytest.mark.parametrize("which", ["restatement", "reference"])
def test_conditions_on_the_inputs(which):
    if which == "reference" and ca.ref_lib() is None:
        pytest.skip("oracle/_ref not built")
    runs = _runs(which == "reference")
    text = "\n".join(L.format_report(name, runs[name]) for name in L.scene_names())
    for name in L.scene_names():
        assert not L.unmet_conditions(runs[name]), text
    for name in ("s28", "s38", "s54"):   # the main scenes: every range they reach is a full class, not a tail
        first = [q for q in runs[name]["report"] if q["round"] == 0]
        assert all(q["hi"] - q["lo"] >= L.TAIL for q in first), text
    assert [q["lo"] for q in runs["s54"]["report"] if q["round"] == 0] == [0, 4096, 8192, 16384]
    # every range above the first has its deciding scenes: first-round rejections that need the range's own accepted bits
    for lo, names in ((4096, ("s28",)), (8192, ("s38", "n16384")), (16384, ("s54",))):
        for name in names:
            q = [q for q in runs[name]["report"] if q["round"] == 0 and q["lo"] == lo][0]
            assert q["own_range"] >= L.MIN_CHAIN_REJECTED, text


@pytest.mark.parametrize("which", ["restatement", "reference"])
def test_fixture_regenerates(which):
    """Every scene again from the generator's parameters and the oracle, against the committed file (which the reference's
    function wrote): parameters, cube, rounds, per-round candidate counts and cluster sizes, the per-range report, the cluster."""
    if which == "reference" and ca.ref_lib() is None:
        pytest.skip("oracle/_ref not built")
    g = np.load(GOLD)
    assert list(g["names"]) == L.scene_names()
    runs = _runs(which == "reference")
    for name in L.scene_names():
        sc, r = L.scene(name), runs[name]
        assert tuple(g[name + "_cube"]) == sc["cube"] and g[name + "_n_shell"] == sc["n_shell"] and g[name + "_n_outer"] == sc["n_outer"]
        assert np.array_equal(g[name + "_seed"], sc["seed"]) and np.array_equal(g[name + "_vertex_idx"], r["vertex_idx"])
        assert g[name + "_iters"] == r["iters"] == L.ROUNDS
        assert np.array_equal(g[name + "_n_cand"], r["n_cand"]), (name, g[name + "_n_cand"], r["n_cand"])
        assert np.array_equal(g[name + "_sizes"], r["sizes"]), (name, g[name + "_sizes"], r["sizes"])
        assert np.array_equal(g[name + "_report"], np.array([[q[c] for c in L.REPORT_COLUMNS] for q in r["report"]], np.int32))
        assert str(g[name + "_sha256"]) == L.cluster_digest(r["cluster"])
        assert g[name + "_cluster"].dtype == np.int32 and np.array_equal(g[name + "_cluster"], r["cluster"])
    assert os.path.getsize(GOLD) < 1 << 20


def test_round_by_round_equals_the_whole_loop():
    """run_scene steps cl_cluster_round; polygon_generation runs the restated polygonGeneration in one piece."""
    sc = L.scene("n4096")
    r = _RUNS[False]["n4096"] if False in _RUNS else L.run_scene(sc)
    v, cl, it, rc = ca.polygon_generation(sc["grid"], sc["seed"], itr_cluster_max=L.ROUNDS)
    assert rc == 0 and it == r["iters"] and np.array_equal(v, r["vertex_idx"]) and np.array_equal(cl, r["cluster"])


def test_side_rooms_leave_the_scene_alone():
    """The rooms the mixed-batch and overflow tests add lie outside the box of the scene's second shell, so the scene's rows
    keep the fixture's answer; the rooms' own seeds give a one-voxel cluster and a small live one."""
    for name in ("s28", "n16384", "n16385"):
        sc = L.scene(name)
        grid, pocket, room = L.with_side_rooms(sc)
        added = np.argwhere((grid == 1) & (sc["grid"] == 0))
        hi = np.array(grid.shape) - 5
        assert ((added < 4) | (added > hi)).any(1).all()
        assert not (sc["grid"] == 1)[(grid == 0)].any()          # nothing of the scene was removed
        x0, x1, y0, y1, z0, z1 = sc["box"]
        assert min(x0, y0, z0) - 2 >= 4 and (np.array([x1, y1, z1]) + 2 <= hi).all()   # the second shell's box
        v, cl, it, rc = ca.polygon_generation(grid, pocket, itr_cluster_max=L.ROUNDS)
        assert rc == 0 and it == 0 and np.array_equal(cl, [pocket])
        v, cl, it, rc = ca.polygon_generation(grid, room, itr_cluster_max=L.ROUNDS)
        assert rc == 0 and it >= 1 and len(cl) > 26 and cl[26][0] == 3, (it, cl)
    sc = L.scene("n4095")
    r = _RUNS[False]["n4095"] if False in _RUNS else L.run_scene(sc)
    v, cl, it, rc = ca.polygon_generation(L.with_side_rooms(sc)[0], sc["seed"], itr_cluster_max=L.ROUNDS)
    assert rc == 0 and np.array_equal(cl, r["cluster"]) and np.array_equal(v, r["vertex_idx"])


def test_chunk_scene_has_both_outcomes():
    c = L.chunk_scene()
    assert 66000 <= len(c["cluster"]) <= 70000 and len(c["cluster"]) > 256 * 256 and len(c["cand"]) == 64
    assert not c["grid"][c["cluster"][:, 0], c["cluster"][:, 1], c["cluster"][:, 2]].any()
    lin = (c["cluster"][:, 0] * 44 + c["cluster"][:, 1]) * 36 + c["cluster"][:, 2]
    assert (np.diff(lin) > 0).all()                                               # storage order
    out = ca.serial_convex_test(ca.lib(), "cl_serial_convex_test", c["cand"], c["cluster"], c["inside"], c["grid"], c["grid"].shape)
    assert min(int(out.sum()), int((out == 0).sum())) >= 8, out
    # ... and chunks 256 and up ALONE decide at least 8 of them: a kernel that dropped those chunks would call them clear
    low = ca.serial_convex_test(ca.lib(), "cl_serial_convex_test", c["cand"], c["cluster"][:256 * 256], c["inside"], c["grid"], c["grid"].shape)
    assert int(((out == 0) & (low == 1)).sum()) >= 8
    if ca.ref_lib() is not None:
        assert np.array_equal(ca.serial_convex_test(ca.ref_lib(), "ref_serial_convex_test", c["cand"], c["cluster"], c["inside"],
                                                    c["grid"], c["grid"].shape), out)
