"""The unknown policy DIRECT_UNKNOWN_OCCUPIED (include/direct_cluster.h, "unknown space as occupied") on the CPU:
direct_amd/csrc/map_close_math.h compiled by g++ as a program that emulates k_scan_close as lane loops
(tests/unknown_policy_harness.py), plain and under the address and undefined-behaviour sanitizers, against a restatement written
from the definition's text on top of the plain and the evidence scan's restatements - byte for byte: grids are bytes and the stats
are counts, there are no tolerances."""
import numpy as np
import pytest

from tests import evidence_harness as eh
from tests import frontier_harness as fh
from tests import grid_path_harness as gh
from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh
from tests import unknown_policy_harness as uh

INFLATES = ((0, 0, 0), (2, 2, 1))
MODES = ("reset", "continue", "adopt")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return uh.build(tmp_path_factory.mktemp("unknown_policy"))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return uh.build(tmp_path_factory.mktemp("unknown_policy_san"), sanitize=True)


@pytest.fixture(scope="module")
def clouds():
    out = sh.clouds()
    out["none"] = out["random"][:0]      # n = 0
    return out


@pytest.fixture(scope="module")
def touched(clouds):
    """the touch grid of every (cloud, range) once, shared and left unchanged"""
    return {(name, r): eh.touch_grid(pts, sh.ORIGIN, r) for name, pts in clouds.items() for r in sh.RANGES}


@pytest.fixture(scope="module")
def state():
    """what a handle may hold before a scan: evidence, a scan grid, a closed map with an open map beside it, and a known grid"""
    rng = np.random.default_rng(5)
    ev = rng.integers(-127, 128, sh.DIMS).astype(np.int8)
    ev[rng.random(sh.DIMS) < 0.5] = 0
    known = (rng.random(sh.DIMS) < 0.3).astype(np.uint8)
    opened = (rng.random(sh.DIMS) < 0.2).astype(np.uint8)
    return dict(ev=ev, raw=(rng.random(sh.DIMS) < 0.5).astype(np.uint8), known=known, open=opened, before=opened | (known == 0).astype(np.uint8))


def properties(w):
    """what the definition promises of every result"""
    kn = w["known"] != 0
    assert np.array_equal(w["map"][kn], w["open"][kn])                              # known voxels agree between map and open map
    assert (w["map"][~kn] == 1).all()                                               # unknown voxels are closed
    assert w["closed"] == w["map"].size - int((kn | (w["open"] == 1)).sum())        # closed == G - |known U open|
    assert w["open_ones"] == int(w["open"].sum()) and w["stats"][5] == int(w["map"].sum()) == w["open_ones"] + w["closed"]
    assert np.array_equal(fh.frontier_voxels(w["map"], w["known"]), fh.frontier_voxels(w["open"], w["known"]))   # min_d2 == 0


@pytest.mark.parametrize("mode", MODES)
def test_plain_scan_program_equals_the_restatement(harness, clouds, touched, state, mode):
    """every cloud and range the scan tests use and n = 0, both inflations, from a handle that holds everything; ADOPT with and
    without an open map"""
    closed = 0
    for name, pts in clouds.items():
        for r in sh.RANGES:
            for k, inflate in enumerate(INFLATES):
                held = state["open"] if k == 0 else None
                w = uh.restate_plain(pts, sh.ORIGIN, r, inflate, mode, state["raw"], state["before"], state["known"], held)
                properties(w)
                uh.same_close(harness, w, state["before"], lanes=(1, 7, 64)[(k + len(pts)) % 3])
                short = uh.restate_plain(pts, sh.ORIGIN, r, inflate, mode, state["raw"], state["before"], state["known"], held,
                                         touched=touched[name, r])           # the shared walks give the same scan
                assert all(np.array_equal(short[key], w[key]) for key in w), (name, r)
                if mode == "adopt" and held is not None:       # unknown voxels do not become returns
                    assert not w["raw"][(state["open"] == 0) & (w["known"] == 0)].any()
                closed += w["closed"]
    assert closed > 0


@pytest.mark.parametrize("mode", MODES)
def test_evidence_scan_program_equals_the_restatement(harness, clouds, touched, state, mode):
    closed = 0
    for name, pts in clouds.items():
        for r in sh.RANGES:
            for k, inflate in enumerate(INFLATES):
                par = (eh.DEFAULTS, eh.SMALL)[k]
                held = state["open"] if k == 0 else None
                w = uh.restate_evidence(pts, sh.ORIGIN, r, par, inflate, mode, state["ev"], state["before"], state["known"], held,
                                        touched=touched[name, r])
                properties(w)
                uh.same_close(harness, w, state["before"], lanes=(64, 3, 256)[(k + len(pts)) % 3])
                if mode == "adopt" and held is not None:
                    assert not w["raw"][(state["open"] == 0) & (w["known"] == 0)].any()
                closed += w["closed"]
    assert closed > 0


def small_map():
    dims, lower = (9, 7, 5), np.array([0.3, -0.45, 0.15])
    upper = lower + np.array(dims) * sh.RES
    origin = lower + np.array([4.3, 3.6, 2.2]) * sh.RES
    pts = np.concatenate([mh.cloud_random(40, dims, sh.RES, lower, seed=4), mh.cloud_borders(dims, sh.RES, lower, upper)])
    return dims, lower, upper, origin, pts


def small_cases():
    """315 voxels (a tail of 11) through both scans and all modes"""
    dims, lower, upper, origin, pts = small_map()
    assert np.prod(dims) % 16 == 11
    kw = dict(dims=dims, lower=lower, upper=upper)
    rng = np.random.default_rng(1)
    ev = rng.integers(-127, 128, dims).astype(np.int8)
    known = (rng.random(dims) < 0.4).astype(np.uint8)
    opened = (rng.random(dims) < 0.3).astype(np.uint8)
    before = opened | (known == 0).astype(np.uint8)
    for mode in MODES:
        for inflate in ((0, 0, 0), (15, 15, 7)):
            yield before, uh.restate_plain(pts, origin, 1.0, inflate, mode, opened, before, known, opened, **kw)
            yield before, uh.restate_evidence(pts, origin, 1.0, eh.SMALL, inflate, mode, ev, before, known, opened, **kw)


def test_a_voxel_count_that_is_no_multiple_of_16(harness):
    seen = 0
    for before, w in small_cases():
        properties(w)
        for lanes in (1, 64):
            uh.same_close(harness, w, before, lanes)
        seen += int((w["map"].ravel()[-11:] != before.ravel()[-11:]).any())
    assert seen > 0                                            # the tail is written


@pytest.mark.parametrize("G", (16, 17, 1, 15, 31, 32, 33))
def test_grids_of_exactly_16_and_17_voxels(harness, sanitized, G):
    """one whole group; one whole group and a tail of one; and their neighbours.  Every combination of the four bytes occurs."""
    rng = np.random.default_rng(G)
    for trial in range(8):
        opened, known, raw = (rng.integers(0, 2, (G, 1, 1)).astype(np.uint8) for _ in range(3))
        known *= rng.integers(1, 256, known.shape).astype(np.uint8)          # known is "!= 0", any byte
        before = rng.integers(0, 3, (G, 1, 1)).astype(np.uint8) if trial else None   # set_map's bytes may be anything
        new, counts = uh.close(opened, known, raw, before)
        for h in (harness, sanitized):
            for lanes in (1, 2, 64):
                got, c, _ = uh.run(h, opened, known, raw, before, lanes)
                assert np.array_equal(got, new) and c.tolist() == counts.tolist(), (G, trial, lanes)


def test_header_program_under_the_sanitizers(sanitized, clouds, touched, state):
    """the same program built with -fsanitize=address,undefined (no recovery: a finding is a non-zero exit), stand-alone; the grids
    are heap buffers of exactly G bytes, so a close pass that read or wrote past the tail would be found"""
    for before, w in small_cases():
        uh.same_close(sanitized, w, before, lanes=3)
    for mode in MODES:
        w = uh.restate_evidence(clouds["random"], sh.ORIGIN, 10.0, eh.SMALL, (2, 2, 1), mode, state["ev"], state["before"], state["known"],
                                state["open"], touched=touched["random", 10.0])
        uh.same_close(sanitized, w, state["before"], lanes=7)


def test_a_scan_that_teaches_nothing_stores_nothing(harness, clouds):
    pts = clouds["random"]
    w1 = uh.restate_plain(pts, sh.ORIGIN, 10.0, (2, 2, 1), "continue")
    assert w1["stats"][6] > 0 and w1["stats"][7] == 0 and w1["stats"][6] == w1["stats"][5]   # from no map: everything is set
    w2 = uh.restate_plain(pts, sh.ORIGIN, 10.0, (2, 2, 1), "continue", w1["raw"], w1["map"], w1["known"], w1["open"])
    assert w2["stats"][6] + w2["stats"][7] == 0 and np.array_equal(w2["map"], w1["map"])
    _, counts, stores = uh.run(harness, w2["open"], w2["known"], w2["raw"], w1["map"])
    assert stores == 0 and counts[2] + counts[3] == 0
    _, _, stores = uh.run(harness, w1["open"], w1["known"], w1["raw"], None)
    assert stores > 0


def test_order_and_launch_shape_do_not_matter(harness, clouds, state):
    pts = np.concatenate([clouds["random"], clouds["lattice"]])
    shuffled = pts[np.random.default_rng(3).permutation(len(pts))]
    a = uh.restate_plain(pts, sh.ORIGIN, 10.0, (2, 2, 1), "continue", state["raw"], state["before"], state["known"])
    b = uh.restate_plain(shuffled, sh.ORIGIN, 10.0, (2, 2, 1), "continue", state["raw"], state["before"], state["known"])
    for k in ("raw", "open", "map", "known", "stats"):
        assert np.array_equal(a[k], b[k]), k
    want = uh.run(harness, a["open"], a["known"], a["raw"], state["before"], 64)
    for lanes in (1, 7, 256, 1000):
        got = uh.run(harness, a["open"], a["known"], a["raw"], state["before"], lanes)
        assert np.array_equal(got[0], want[0]) and got[1].tolist() == want[1].tolist()


def test_policy_values_and_the_scan_refusal(harness):
    assert [uh.policy_known(harness, v) for v in (-1, 0, 1, 2, 255)] == [False, True, True, False, False]
    assert uh.refusal(harness, uh.FREE, 0) == "ok" and uh.refusal(harness, uh.FREE, 1) == "ok" and uh.refusal(harness, uh.OCCUPIED, 1) == "ok"
    assert "DIRECT_SCAN_TRACK_KNOWN" in uh.refusal(harness, uh.OCCUPIED, 0)


def test_the_free_path_of_the_l_scene_crosses_unknown_space(tmp_path):
    """the scene of tests/test_gpu_unknown_policy.py, checked here without a GPU by the Dijkstra of tests/grid_path_harness.py: on
    the open map (empty) the cheapest path between the far ends of the L leaves the known region; on the closed bytes it stays
    inside and is longer, and the island is out of reach"""
    sc = uh.l_scene()
    known = sc["known"]
    arms = (known[4:7, 4:32, 4:7], known[4:36, 29:32, 4:7])
    assert all(a.all() and min(a.shape) == 3 and max(a.shape) >= 12 for a in arms)
    assert known[sc["start"]] == 1 and known[sc["goal"]] == 1 and known[sc["island_goal"]] == 1
    opened = np.zeros(sh.DIMS, np.uint8)
    new, _ = uh.close(opened, known, opened, None)
    g = gh.build(tmp_path)
    free = uh.dijkstra(g, opened, [sc["start"]], [sc["goal"]])
    shut = uh.dijkstra(g, new, [sc["start"], sc["start"]], [sc["goal"], sc["island_goal"]])
    assert free["rtn"][0] == gh.OK and any(known[tuple(v)] == 0 for v in free["paths"][0])
    assert shut["rtn"].tolist() == [gh.OK, gh.NO_PATH] and all(known[tuple(v)] == 1 for v in shut["paths"][0])
    assert shut["path_cost"][0] > free["path_cost"][0]
