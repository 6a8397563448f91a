"""The arithmetic of direct_cluster_plan_check_batch on the CPU: direct_amd/csrc/plan_check_math.h's pruned descent (compiled by g++,
tests/plan_check_harness.py) against a NumPy restatement of the header text that visits every leaf.  Nothing here has a tolerance:
outputs are compared integer for integer and bit for bit, and the soundness test checks exact voxel membership."""
import itertools
import os

import numpy as np
import pytest

from tests import plan_check_harness as ph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEPTHS = (0, 1, 5, 7)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ph.build(tmp_path_factory.mktemp("plan_check"))


@pytest.fixture(scope="module")
def grid():
    return ph.shared_map()


@pytest.fixture(scope="module")
def inputs():
    return ph.shared_inputs()


@pytest.fixture(scope="module")
def crafted_out(grid):
    """the crafted rows at their depth, from bez: (outside_blocks, t_from used) -> outputs"""
    c = ph.pick(ph.crafted(), "bez")
    return {(ob, tf): ph.restate(c, grid, ph.CRAFTED_DEPTH, outside_blocks=ob, use_t_from=tf) for ob in (False, True) for tf in (False, True)}


def row(name):
    return ph.CRAFTED.index(name)


def test_map_has_a_few_dozen_blocks(grid):
    assert grid.shape == (40, 36, 12) and 100 < int(grid.sum()) < grid.size // 4


@pytest.mark.parametrize("name", ["random7", "crafted", "long5", "invalid9"])
@pytest.mark.parametrize("kind", ["bez", "poly"])
def test_descent_equals_every_leaf(harness, grid, inputs, name, kind):
    inp = ph.pick(inputs[name], kind)
    pairs = 0
    for depth, (margin, ob, tf) in itertools.product(DEPTHS if name != "long5" else (0, 6), ((0.0, False, True), (0.2, True, False), (0.0, True, True))):
        want = ph.restate(inp, grid, depth, margin, ob, tf)
        got, info = ph.run(harness, inp, grid, depth, margin, ob, tf)
        ph.assert_same(got, want, f"{name} {kind} D={depth} margin={margin} outside={ob} t_from={tf}")
        assert info["not_nested"] == 0, info   # nesting: every visited child's index box lies inside its parent's
        pairs += info["pairs"]
    assert pairs > 0


def test_float_rounded_inputs(harness, grid, inputs):
    inp = ph.as_f32(ph.pick(inputs["random7"], "poly"))
    want = ph.restate(inp, grid, 6)
    got, _ = ph.run(harness, inp, grid, 6)
    ph.assert_same(got, want, "float32 storage")


@pytest.mark.parametrize("name", ["random7", "crafted", "long5"])
@pytest.mark.parametrize("ob", [False, True])
def test_sound_before_t_free(grid, inputs, name, ob):
    """the dyadic points of depth D + 3 with times in [t_from, t_free) lie in voxels with byte 0 (and, with outside_blocks, inside the map)"""
    depth = 4
    inp = ph.pick(inputs[name], "bez")
    out = ph.restate(inp, grid, depth, outside_blocks=ob)
    checked = 0
    for b in np.flatnonzero(out["status"] == 0):
        t, p = ph.dyadic(inp, b, depth + 3)
        sel = (t >= inp["t_from"][b]) & (t < out["t_free"][b])
        assert not ph.voxel_bytes(p[sel], grid).any(), (name, b)
        if ob:
            q = (p[sel] - ph.LOWER) * (1.0 / ph.RES)
            assert ((q >= 0) & (q < np.array(grid.shape))).all(), (name, b)
        checked += int(sel.sum())
    assert checked > 0


def test_coverage_free_and_blocked_rows(crafted_out):
    o = crafted_out[(False, False)]
    assert (o["status"] == 0).all()
    r = row("free")
    assert o["verdict"][r] == 0 and tuple(o["first"][r]) == (-1, -1) and o["t_free"][r] == 2.0 and (o["hit_box"][r] == -1).all()
    assert o["verdict"][row("leaf0")] == 1 and tuple(o["first"][row("leaf0")]) == (0, 0) and o["t_free"][row("leaf0")] == 0.0
    last = (1 << ph.CRAFTED_DEPTH) - 1
    assert tuple(o["first"][row("lastleaf")]) == (0, last) and o["t_free"][row("lastleaf")] == last / 32.0
    r = row("later")
    assert o["first"][r][0] == 2 and (o["seg_first"][r][:2] == -1).all() and o["seg_first"][r][2] >= 0 and 2.0 <= o["t_free"][r] < 3.0


def test_coverage_t_from(crafted_out):
    a, b = crafted_out[(False, False)], crafted_out[(False, True)]
    r = row("from_later")
    assert a["first"][r][0] == 0 and b["first"][r][0] == 2 and b["verdict"][r] == 1 and b["t_free"][r] > a["t_free"][r]
    r = row("from_free")
    assert a["verdict"][r] == 1 and b["verdict"][r] == 0 and b["t_free"][r] == 3.0
    others = [i for i, k in enumerate(ph.CRAFTED) if not k.startswith("from_")]
    for k in ph.KEYS:
        assert np.array_equal(a[k][others], b[k][others])


def test_coverage_map_border(crafted_out):
    off, on = crafted_out[(False, False)], crafted_out[(True, False)]
    r = row("leaving")
    assert off["verdict"][r] == 0 and on["verdict"][r] == 2 and on["first"][r][0] == 0 and on["hit_box"][r][0] == -1
    assert on["hit_box"][r][3] >= 0                                     # that leaf straddles the face
    r = row("outside")
    assert off["verdict"][r] == 0 and on["verdict"][r] == 2 and tuple(on["first"][r]) == (0, 0)
    assert on["hit_box"][r][0] == -1 and on["hit_box"][r][3] == -1        # a box wholly outside the map: never occupied


def test_coverage_conservative_row(grid):
    c = ph.pick(ph.crafted(), "bez")
    r = row("conservative")
    o2 = ph.restate(c, grid, 2, use_t_from=False)
    assert o2["verdict"][r] == 1 and tuple(o2["first"][r]) == (0, 0)
    _, p = ph.dyadic(c, r, 2 + 3)
    assert not ph.voxel_bytes(p, grid).any()                            # blocked, yet no dense point lies in an occupied voxel
    assert ph.restate(c, grid, ph.CRAFTED_DEPTH, use_t_from=False)["verdict"][r] == 0   # and a deeper check clears it


def test_coverage_margin(grid):
    c = ph.pick(ph.crafted(), "bez")
    r = row("margin")
    assert ph.restate(c, grid, ph.CRAFTED_DEPTH, margin=0.0, use_t_from=False)["verdict"][r] == 0
    assert ph.restate(c, grid, ph.CRAFTED_DEPTH, margin=0.2, use_t_from=False)["verdict"][r] == 1


def test_coverage_invalid_rows(grid, inputs):
    for kind in ("bez", "poly"):
        o = ph.restate(ph.pick(inputs["invalid9"], kind), grid, 5)
        bad = sorted(ph.INVALID_ROWS)
        good = [b for b in range(9) if b not in bad]
        assert (o["status"][bad] == -1).all() and (o["verdict"][bad] == ph.INVALID).all() and (o["t_free"][bad] == 0).all()
        assert (o["first"][bad] == -1).all() and (o["hit_box"][bad] == -1).all() and (o["seg_first"][bad] == -1).all()
        assert (o["status"][good] == 0).all() and (o["verdict"][good] >= 0).all()


def test_bez_and_poly_agree_away_from_faces(grid, inputs):
    """the same curves from bez and from poly: equal verdicts wherever no edge of a judged box lies within 1e-9 of a voxel face"""
    compared = 0
    for name in ("random7", "crafted", "long5"):
        inp = inputs[name]
        ob, op = (ph.restate(ph.pick(inp, k), grid, 5, use_t_from=False) for k in ("bez", "poly"))
        for b in range(len(inp["n_seg"])):
            near = False
            for i in range(int(inp["n_seg"][b])):
                L = ph.leaves(ph.control_points(inp["bez"][b, i], inp["T"][b, i], False), 5)
                q = (np.stack([L.min(axis=2), L.max(axis=2)]) - ph.LOWER) * (1.0 / ph.RES)
                near = near or bool((np.abs(q - np.rint(q)) * ph.RES < 1e-9).any())
            if not near:
                assert ob["verdict"][b] == op["verdict"][b] and tuple(ob["first"][b]) == tuple(op["first"][b]), (name, b)
                compared += 1
    assert compared >= 10


def test_solved_plan_blocked_at_pinned_leaf(harness):
    """a solved plan (tests/golden/free_n5.npz, row 0) on an empty map with one block on its path"""
    g = np.load(os.path.join(GOLDEN, "free_n5.npz"))
    inp = dict(n_seg=g["n_seg"][:1], T=g["p0_T"][:1], poly=g["p0_poly"][:1])
    t, p = ph.dyadic(inp, 0, 4)
    lower = np.floor(p.min(axis=0)) - 1.0
    dims = tuple(int(v) for v in np.ceil((p.max(axis=0) + 1.0 - lower) / ph.RES))
    S = ph.starts(inp["T"][0], int(inp["n_seg"][0]))
    mid = p[np.argmin(np.abs(t - (S[2] + 0.5 * inp["T"][0, 2])))]       # the middle of segment 2
    v = np.trunc((mid - lower) / ph.RES).astype(int)
    grid = np.zeros(dims, np.uint8)
    assert ph.restate(inp, grid, 6, lower=lower)["verdict"][0] == 0
    grid[v[0], v[1], v[2]] = 1
    want = ph.restate(inp, grid, 6, lower=lower)
    got, _ = ph.run(harness, inp, grid, 6, lower=lower)
    ph.assert_same(got, want, "solved plan")
    assert want["verdict"][0] == 1 and want["first"][0][0] == 2
    lo, hi = want["hit_box"][0][:3], want["hit_box"][0][3:]
    assert (lo <= v).all() and (v <= hi).all()
    print("first blocked leaf", tuple(want["first"][0]), "t_free", want["t_free"][0])
    assert tuple(want["first"][0]) == PINNED_LEAF


PINNED_LEAF = (2, 30)   # the block sits at the middle of segment 2 (leaf 32 of 64); the curve's boxes reach its voxel two leaves earlier
