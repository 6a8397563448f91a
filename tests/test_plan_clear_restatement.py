"""direct_amd/csrc/plan_clear_math.h compiled by g++ against the NumPy restatement of tests/dist_field_harness.py, which evaluates
every leaf: every integer and every bit of the doubles.  Then the bound itself against a yardstick independent of both: the exact
distance of densely sampled curve points to the union of the occupied voxel cubes.  No GPU."""
import numpy as np
import pytest

from tests import dist_field_harness as dh
from tests import plan_check_harness as ph


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("plan_clear"))


@pytest.fixture(scope="module")
def grid():
    return ph.shared_map()


@pytest.fixture(scope="module")
def fields(grid):
    exact = dh.brute_d2(grid)
    return {cap: np.minimum(exact, dh.cap2_of(cap)).astype(np.int32) for cap in (0, 4)}


@pytest.fixture(scope="module")
def inputs():
    return dh.clear_inputs()


def test_the_constant():
    """K is the smallest double not below sqrt(3)/2: K^2 >= 3/4 > (the double below K)^2, in exact rational arithmetic"""
    from fractions import Fraction
    below = np.nextafter(dh.K, 0.0)
    assert Fraction(dh.K) ** 2 >= Fraction(3, 4) > Fraction(float(below)) ** 2
    assert dh.K == 0.8660254037844387


@pytest.mark.parametrize("depth", [0, 1, 5, 6, 7])
def test_header_equals_the_restatement(harness, fields, inputs, depth):
    for name in ("random7", "crafted", "invalid9", "leaving1", "long5"):
        for kind, f32, use_t_from, radius in dh.COMBOS:
            inp = ph.pick(inputs[name], kind)
            inp = ph.as_f32(inp) if f32 else inp
            for cap in ((0, 4) if name == "random7" else (0,)):
                want = dh.restate_clearance(inp, fields[cap], depth, radius, use_t_from)
                got = dh.run_clear(harness, inp, fields[cap], depth, radius, use_t_from)
                dh.assert_same(got, want, f"{name} D={depth} {kind} f32={f32} t_from={use_t_from} radius={radius} cap={cap}")


def test_the_inputs_reach_every_branch(fields, inputs):
    """box centres outside the map, rows with and without a leaf below the radius, a row without a judged leaf, invalid rows"""
    out = dh.restate_clearance(ph.pick(inputs["leaving1"], "bez"), fields[0], 6, 0.3)
    assert out["status"][0] == 0 and not out["centre_inside"][0] and out["clearance"][0] < -1.0   # ~4 m outside: nothing certified
    out = dh.restate_clearance(ph.pick(inputs["random7"], "bez"), fields[0], 6, 0.3)
    assert set(out["verdict"]) == {0, 1}
    assert np.isinf(out["clearance"][6]) and (out["where"][6] == -1).all() and out["t_min"][6] == out["t_free"][6]   # t_from past the end
    assert (out["seg_clearance"][1, 1:] != out["seg_clearance"][1, 1:]).all()     # past n_seg = 1
    out = dh.restate_clearance(ph.pick(inputs["invalid9"], "bez"), fields[0], 5, 0.3)
    bad = sorted(ph.INVALID_ROWS)
    assert (out["status"][bad] == -1).all() and (out["verdict"][bad] == dh.INVALID).all() and np.isnan(out["clearance"][bad]).all()
    assert (out["t_min"][bad] == 0).all() and (out["t_free"][bad] == 0).all() and (out["where"][bad] == -1).all()
    empty = np.full(fields[0].shape, dh.NONE, np.int32)
    out = dh.restate_clearance(ph.pick(inputs["crafted"], "bez"), empty, 5, 0.3, use_t_from=False)
    assert np.isinf(out["clearance"]).all() and (out["verdict"] == 0).all() and (out["where"] == -1).all()


def test_a_capped_field_never_raises_the_bound(fields, inputs):
    inp = ph.pick(inputs["random7"], "bez")
    a, b = dh.restate_clearance(inp, fields[0], 6), dh.restate_clearance(inp, fields[4], 6)
    ok = a["status"] == 0
    assert (b["clearance"][ok] <= a["clearance"][ok]).all() and (b["clearance"][ok] < a["clearance"][ok]).any()


@pytest.fixture(scope="module")
def true_distance(grid, inputs):
    """per input set and valid row: (times, exact distance to the occupied cubes) of the curve points at depth 10"""
    out = {}
    for name in ("random7", "crafted"):
        inp = ph.pick(inputs[name], "bez")
        for b in range(len(inp["n_seg"])):
            t, p = ph.dyadic(inp, b, 10)
            out[name, b] = (t, dh.cube_distance(p, grid))
    return out


@pytest.mark.parametrize("depth", [2, 6])
@pytest.mark.parametrize("use_t_from", [True, False])
def test_the_bound_is_sound_and_tight(grid, fields, inputs, true_distance, depth, use_t_from):
    """SOUND: no sampled curve point of the judged span is closer to an occupied cube than the certified clearance (1e-9 m for the
    rounding of the yardstick).  TIGHT: for a row whose minimising leaf has its box centre inside the map, a point of that leaf
    is within bound + 2 half + 2 off + K res of the cubes (the triangle inequality the other way round, off <= sqrt(3)/2 res), so
    the sampled minimum is at most clearance + 2 half_max + 1.5 sqrt(3) res; a bound of minus infinity would fail here."""
    checked = tight = 0
    for name in ("random7", "crafted"):
        inp = ph.pick(inputs[name], "bez")
        out = dh.restate_clearance(inp, fields[0], depth, 0.0, use_t_from)
        assert (out["status"] == 0).all()
        for b in range(len(inp["n_seg"])):
            t, dist = true_distance[name, b]
            span = t > inp["t_from"][b] if use_t_from else np.ones(len(t), bool)
            if not span.any():
                assert np.isinf(out["clearance"][b])
                continue
            least = dist[span].min()
            assert least >= out["clearance"][b] - 1e-9, f"{name} row {b}: a curve point at {least} m, certified {out['clearance'][b]} m"
            checked += 1
            if out["centre_inside"][b]:
                assert least <= out["clearance"][b] + 2 * out["half_max"][b] + 1.5 * np.sqrt(3.0) * ph.RES + 1e-9, f"{name} row {b}"
                tight += 1
    assert checked >= 14 and tight >= 10
