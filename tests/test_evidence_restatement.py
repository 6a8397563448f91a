"""Occupancy evidence per voxel (include/direct_cluster.h, "occupancy evidence per voxel") on the CPU:
direct_amd/csrc/map_evidence_math.h and map_scan_math.h compiled by g++ as a program that emulates the three kernels as lane loops
(tests/evidence_harness.py), plain and under the address and undefined-behaviour sanitizers, against a restatement written from the
definition's text - byte for byte: grids are bytes and stats are counts, there are no tolerances.  The plain scan is the special
case (hit, miss, ev_min, ev_max, occ) = (1, 1, 0, 1, 1), which pins the new code against tests/map_scan_harness.py."""
import math

import numpy as np
import pytest

from tests import evidence_harness as eh
from tests import frontier_harness as fh
from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh

INFLATES = ((0, 0, 0), (2, 2, 1))
PARAMS = (eh.DEFAULTS, eh.SMALL)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return eh.build(tmp_path_factory.mktemp("evidence"))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return eh.build(tmp_path_factory.mktemp("evidence_san"), sanitize=True)


@pytest.fixture(scope="module")
def clouds():
    return sh.clouds()


@pytest.fixture(scope="module")
def touched(clouds):
    """the touch grid of every (cloud, range) once, shared by the tests below and left unchanged"""
    return {(name, r): eh.touch_grid(pts, sh.ORIGIN, r) for name, pts in clouds.items() for r in sh.RANGES}


@pytest.fixture(scope="module")
def state():
    """what a handle may hold before a call: evidence over the whole int8 range that can be stored, a map, a scan grid that
    disagrees with the evidence, and a known grid"""
    rng = np.random.default_rng(5)
    ev = rng.integers(-127, 128, sh.DIMS).astype(np.int8)
    ev[rng.random(sh.DIMS) < 0.5] = 0
    return dict(ev=ev, before=(rng.random(sh.DIMS) < 0.2).astype(np.uint8), raw=(rng.random(sh.DIMS) < 0.5).astype(np.uint8),
                known=(rng.random(sh.DIMS) < 0.3).astype(np.uint8))


def passed_and_hit(pts, max_range):
    """-> (voxels that one ray ends in and another passes, hit voxels)"""
    passed, hit = np.zeros(sh.DIMS, bool), np.zeros(sh.DIMS, bool)
    inv = 1.0 / sh.RES
    for p in pts:
        kind, cleared, _ = sh.walk(p, sh.ORIGIN, max_range)
        for v in cleared:
            passed[v] = True
        if kind == sh.HIT:
            j = tuple(int(math.floor((float(p[a]) - float(sh.LOWER[a])) * inv)) for a in range(3))
            if all(0 <= j[a] < sh.DIMS[a] for a in range(3)):
                hit[j] = True
    return int((passed & hit).sum()), int(hit.sum())


def test_the_clouds_have_voxels_both_passed_and_hit(clouds, touched):
    """the figures of the issue, so that 'a hit beats a pass' is not tested vacuously"""
    assert passed_and_hit(clouds["random"], 10.0) == (244, 454)
    assert passed_and_hit(clouds["lattice"], 10.0) == (475, 1078)
    assert passed_and_hit(clouds["random"], 1.5) == (60, 70)
    assert int((touched["random", 10.0][0] == 2).sum()) == 454 and int((touched["lattice", 10.0][0] == 2).sum()) == 1078


@pytest.mark.parametrize("max_range", sh.RANGES)
@pytest.mark.parametrize("mode", ("reset", "continue", "adopt"))
def test_header_program_equals_the_restatement(harness, clouds, touched, state, mode, max_range):
    """every cloud, both inflations, both parameter sets, tracked and untracked, both strides, from a handle that holds something"""
    seen_hits = 0
    for name, pts in clouds.items():
        for inflate in INFLATES:
            for k, par in enumerate(PARAMS):
                track = bool(k) ^ (inflate == INFLATES[0])
                want = eh.restate(pts, sh.ORIGIN, max_range, par, inflate, mode, state["ev"], state["before"], state["known"], track,
                                  touched=touched[name, max_range])
                cloud = pts if k == 0 else mh.with_stride4(pts)
                got = eh.run(harness, cloud, sh.ORIGIN, max_range, par, inflate, mode, state["ev"], state["raw"], state["before"],
                             state["known"], track)
                eh.same(got, want)
                assert np.array_equal(got["raw"], (got["ev"].astype(np.int32) >= par["occ"]).astype(np.uint8))
                seen_hits += int(want["stats"][8])
    assert seen_hits > 0


def test_header_program_under_the_sanitizers(sanitized, clouds, touched, state):
    """the same program built with -fsanitize=address,undefined (no recovery: a finding is a non-zero exit), stand-alone; the grids
    are buffers of exactly G bytes, so a fold that read or wrote past the tail would be found"""
    for r in sh.RANGES:
        for name, pts in clouds.items():
            for mode, par, inflate in (("continue", eh.SMALL, (2, 2, 1)), ("adopt", eh.DEFAULTS, (0, 0, 0))):
                want = eh.restate(pts, sh.ORIGIN, r, par, inflate, mode, state["ev"], state["before"], state["known"], True, touched=touched[name, r])
                got = eh.run(sanitized, pts, sh.ORIGIN, r, par, inflate, mode, state["ev"], state["raw"], state["before"], state["known"], True,
                             lanes=7)
                eh.same(got, want)
    dims, lower, upper, origin, pts = small_map()
    for mode in ("reset", "continue", "adopt"):
        kw = dict(dims=dims, lower=lower, upper=upper)
        before = np.ones(dims, np.uint8)
        want = eh.restate(pts, origin, 1.0, eh.SMALL, (15, 15, 7), mode, None, before, None, True, **kw)
        eh.same(eh.run(sanitized, pts, origin, 1.0, eh.SMALL, (15, 15, 7), mode, before=before, track=True, lanes=3, **kw), want)


def plain_sequence(scans, inflate, raw=None, before=None, known=None):
    """the plain tracked scans of tests/map_scan_harness.py and tests/frontier_harness.py, one after the other"""
    out = []
    for pts, r in scans:
        raw, before, stats = sh.restate(pts, sh.ORIGIN, r, inflate, raw=raw, before=before)
        known = fh.known_restate(pts, sh.ORIGIN, r, known)
        out.append((raw, before, known, stats))
    return out


@pytest.mark.parametrize("inflate", INFLATES)
def test_the_plain_scan_is_a_special_case(harness, clouds, inflate):
    """(hit, miss, ev_min, ev_max, occ) = (1, 1, 0, 1, 1) is 'the last observation wins': scan grid, map, known grid and
    stats[0..7] equal the plain scan's restatement after RESET, after ADOPT of a full map and over three CONTINUE scans"""
    pts = clouds["random"]
    scans = ((pts[:400], 10.0), (pts[400:700], 1.5), (np.concatenate([pts[700:], clouds["lattice"]]), 10.0))
    # RESET on a handle that held a map
    old = (np.random.default_rng(2).random(sh.DIMS) < 0.3).astype(np.uint8)
    (raw, new, known, stats), = plain_sequence(scans[:1], inflate, before=old)
    for program in (False, True):
        got = (eh.run(harness, scans[0][0], sh.ORIGIN, 10.0, eh.LAST_WINS, inflate, "reset", before=old, track=True) if program else
               eh.restate(scans[0][0], sh.ORIGIN, 10.0, eh.LAST_WINS, inflate, "reset", before=old, track=True))
        assert np.array_equal(got["raw"], raw) and np.array_equal(got["map"], new) and np.array_equal(got["known"], known)
        assert got["stats"][:8].tolist() == stats.tolist() and np.array_equal(got["ev"], raw.astype(np.int8))
    # ADOPT of a full map
    full = np.ones(sh.DIMS, np.uint8)
    (raw, new, known, stats), = plain_sequence(scans[:1], inflate, raw=full, before=full)
    for program in (False, True):
        got = (eh.run(harness, scans[0][0], sh.ORIGIN, 10.0, eh.LAST_WINS, inflate, "adopt", before=full, track=True) if program else
               eh.restate(scans[0][0], sh.ORIGIN, 10.0, eh.LAST_WINS, inflate, "adopt", before=full, track=True))
        assert np.array_equal(got["raw"], raw) and np.array_equal(got["map"], new) and np.array_equal(got["known"], known)
        assert got["stats"][:8].tolist() == stats.tolist() and stats[7] > 0
    # three CONTINUE scans on a handle that held nothing
    for program in (False, True):
        ev = before = known = None
        for (pts_k, r), (raw, new, kn, stats) in zip(scans, plain_sequence(scans, inflate)):
            got = (eh.run(harness, pts_k, sh.ORIGIN, r, eh.LAST_WINS, inflate, "continue", ev, None, before, known, True) if program else
                   eh.restate(pts_k, sh.ORIGIN, r, eh.LAST_WINS, inflate, "continue", ev, before, known, True))
            assert np.array_equal(got["raw"], raw) and np.array_equal(got["map"], new) and np.array_equal(got["known"], kn)
            assert got["stats"][:8].tolist() == stats.tolist()
            ev, before, known = got["ev"], got["map"], got["known"]


def test_order_and_launch_shape_do_not_matter(harness, clouds, state):
    pts = np.concatenate([clouds["random"], clouds["lattice"]])
    kw = dict(par=eh.SMALL, inflate=(2, 2, 1), mode="continue", ev=state["ev"], raw=state["raw"], before=state["before"], known=state["known"],
              track=True)
    want = eh.run(harness, pts, sh.ORIGIN, 10.0, lanes=64, **kw)
    assert want["stats"][8] > 0
    rng = np.random.default_rng(3)
    shuffled = pts[rng.permutation(len(pts))]
    for lanes in (1, 7, 64, 256, (len(pts) + 1) // 2):    # the last: the cloud split in two calls' worth of lanes
        for cloud in (pts, shuffled):
            eh.same(eh.run(harness, cloud, sh.ORIGIN, 10.0, lanes=lanes, **kw), want)
    doubled = eh.run(harness, np.concatenate([pts, shuffled]), sh.ORIGIN, 10.0, lanes=7, **kw)   # a voxel is updated once per scan
    eh.same(doubled, want, ("ev", "raw", "map", "known"))
    assert doubled["stats"][8:].tolist() == want["stats"][8:].tolist() and doubled["stats"][0] == 2 * want["stats"][0]


def test_counting(harness):
    """a wall enters the map at scan ceil(occ / hit) = 2, saturates at ev_max, and once gone leaves after exactly
    ev_max - occ + 1 pass-only scans; a single phantom return never enters; ev_min bounds the free side"""
    par = eh.SMALL
    wpts, room, wall = sh.wall_and_room()
    w = tuple(wall.T)
    both = np.concatenate([wpts, room])
    ev = before = None
    for k in range(1, 6):
        got = eh.run(harness, both, sh.ORIGIN, 10.0, par, mode="continue", ev=ev, before=before)
        eh.same(got, eh.restate(both, sh.ORIGIN, 10.0, par, mode="continue", ev=ev, before=before), ("ev", "raw", "map", "stats"))
        ev, before = got["ev"], got["map"]
        assert (ev[w] == min(2 * k, par["ev_max"])).all()
        assert before[w].all() == (k >= 2) and before[w].any() == (k >= 2)     # at scan 2, not before
    assert (ev[w] == par["ev_max"]).all() and ev.min() == par["ev_min"]        # both limits reached
    for k in range(1, par["ev_max"] - par["occ"] + 2):                         # the wall is gone: the room's rays pass its voxels
        cloud = np.concatenate([room, sh.LOWER + (np.array([[10, 5, 3]]) + 0.5) * sh.RES]).astype(np.float32) if k == 1 else room
        got = eh.run(harness, cloud, sh.ORIGIN, 10.0, par, mode="continue", ev=ev, before=before)
        eh.same(got, eh.restate(cloud, sh.ORIGIN, 10.0, par, mode="continue", ev=ev, before=before), ("ev", "raw", "map", "stats"))
        ev, before = got["ev"], got["map"]
        assert (ev[w] == par["ev_max"] - k).all()
        assert before[w].all() == (k < par["ev_max"] - par["occ"] + 1) and before[w].any() == before[w].all()
        assert before[10, 5, 3] == 0                                           # one return (hit = 2 < occ = 3) never enters the map
    assert ev[10, 5, 3] < par["occ"] and ev.min() == par["ev_min"] and not before[w].any()


def test_untouched_voxels_keep_values_outside_the_clamp(harness):
    par = dict(hit=2, miss=1, ev_min=-3, ev_max=5, occ=3)
    wpts, room, wall = sh.wall_and_room()
    both = np.concatenate([wpts, room])
    rng = np.random.default_rng(9)
    ev = rng.choice(np.array([-128, -127, -90, -4, 0, 1, 4, 6, 90, 127], np.int8), sh.DIMS)
    stored = np.maximum(ev, -127).astype(np.int8)                              # set_evidence: -128 is stored as -127
    got = eh.run(harness, both, sh.ORIGIN, 10.0, par, mode="continue", ev=stored)
    want = eh.restate(both, sh.ORIGIN, 10.0, par, mode="continue", ev=stored)
    eh.same(got, want, ("ev", "raw", "map", "stats"))
    t = want["touch"]
    assert (t == 0).any() and (t == 1).any() and (t == 2).any()
    assert np.array_equal(got["ev"][t == 0], stored[t == 0]) and (np.abs(stored[t == 0].astype(int)) > 5).any()
    s = stored.astype(int)
    assert np.array_equal(got["ev"][t == 2], np.minimum(s[t == 2] + 2, 5)) and np.array_equal(got["ev"][t == 1], np.maximum(s[t == 1] - 1, -3))
    # no points, CONTINUE, another occ: every voxel is thresholded again and the evidence stays
    for occ in (1, 5):
        again = eh.run(harness, both[:0], sh.ORIGIN, 10.0, dict(par, occ=occ), mode="continue", ev=got["ev"], raw=got["raw"], before=got["map"])
        assert np.array_equal(again["ev"], got["ev"]) and np.array_equal(again["raw"], (got["ev"].astype(int) >= occ).astype(np.uint8))
        assert np.array_equal(again["map"], again["raw"]) and again["stats"][8] == 0 and again["stats"][9] == 0
        assert again["stats"][6] + again["stats"][7] == int((again["raw"] != got["raw"]).sum()) > 0


def small_map():
    dims, lower = (9, 7, 5), np.array([0.3, -0.45, 0.15])
    upper = lower + np.array(dims) * sh.RES
    origin = lower + np.array([4.3, 3.6, 2.2]) * sh.RES
    pts = np.concatenate([mh.cloud_random(40, dims, sh.RES, lower, seed=4), mh.cloud_borders(dims, sh.RES, lower, upper)])
    return dims, lower, upper, origin, pts


def test_a_voxel_count_that_is_no_multiple_of_16(harness):
    """9 x 7 x 5 = 315 voxels: the fold's last group has 11"""
    dims, lower, upper, origin, pts = small_map()
    assert np.prod(dims) % 16 == 11
    kw = dict(dims=dims, lower=lower, upper=upper)
    rng = np.random.default_rng(1)
    ev = rng.integers(-127, 128, dims).astype(np.int8)
    before = (rng.random(dims) < 0.4).astype(np.uint8)
    for mode in ("reset", "continue", "adopt"):
        for inflate in ((0, 0, 0), (15, 15, 7)):
            for lanes in (1, 64):
                want = eh.restate(pts, origin, 1.0, eh.SMALL, inflate, mode, ev, before, before, True, **kw)
                got = eh.run(harness, pts, origin, 1.0, eh.SMALL, inflate, mode, ev, 1 - before, before, before, True, lanes=lanes, **kw)
                eh.same(got, want)
                assert want["touch"].ravel()[-11:].any()                       # the tail is touched


def test_parameter_refusals_in_their_order(harness):
    """me::refusal, the function the library calls behind the plain scan's refusals: hit, miss, ev_min, ev_max, occ, reserved, each
    case wrong in one way beyond those behind it in the order"""
    assert eh.refusal(harness, **eh.DEFAULTS) == "ok" and eh.refusal(harness, **eh.SMALL) == "ok" and eh.refusal(harness, **eh.LAST_WINS) == "ok"
    assert eh.refusal(harness, 127, 127, -127, 127, 127) == "ok" and eh.refusal(harness, 1, 1, 0, 1, 1) == "ok"
    for args, word in (((0, 0, 1, 0, 0, (1, 0, 0)), "hit"), ((128, 0, 1, 0, 0, (1, 0, 0)), "hit"),
                       ((1, 0, 1, 0, 0, (1, 0, 0)), "miss"), ((1, 128, 1, 0, 0, (1, 0, 0)), "miss"),
                       ((1, 1, 1, 0, 0, (1, 0, 0)), "ev_min"), ((1, 1, -128, 0, 0, (1, 0, 0)), "ev_min"),
                       ((1, 1, 0, 0, 0, (1, 0, 0)), "ev_max"), ((1, 1, 0, 128, 0, (1, 0, 0)), "ev_max"),
                       ((1, 1, 0, 5, 0, (1, 0, 0)), "occ"), ((1, 1, 0, 5, 6, (1, 0, 0)), "occ"),
                       ((1, 1, 0, 5, 5, (1, 0, 0)), "reserved"), ((1, 1, 0, 5, 5, (0, 0, -1)), "reserved")):
        msg = eh.refusal(harness, *args)
        assert msg.startswith(word + " "), (args, msg)
