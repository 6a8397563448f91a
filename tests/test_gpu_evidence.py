"""direct_cluster_map_integrate_scan_evidence / get_evidence / set_evidence (include/direct_cluster.h, "occupancy evidence per
voxel"; kernels in direct_amd/csrc/map_evidence.h) on the device against the restatement of tests/evidence_harness.py (held equal to
the g++ build of the same headers by tests/test_evidence_restatement.py) and, for the special case (1, 1, 0, 1, 1), against the plain
tracked scan on a second handle.  Grids are bytes and stats are counts: everything is compared for equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import evidence_harness as eh
from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh
from tests import plan_check_harness as ph

pytestmark = pytest.mark.gpu
ROOT = sh.ROOT
SMALL = dict(max_batch=4, cluster_capacity=64, candidate_capacity=64)
INFLATES = ((0, 0, 0), (2, 2, 1))


@pytest.fixture(scope="module")
def gen(built):
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cases():
    """(name, points, range, touch grid) once: n below, at and above one wave and several workgroups of the random cloud, and the
    lattice, at the three ranges; shared and left unchanged"""
    clouds = sh.clouds()
    out = []
    for n in (0, 1, 63, 64, 65, 1000):
        for r in sh.RANGES if n == 1000 else (1.5,):
            out.append(("random_%d" % n, clouds["random"][:n], r))
    out += [("lattice", clouds["lattice"], r) for r in sh.RANGES]
    return [(name, pts, r, eh.touch_grid(pts, sh.ORIGIN, r)) for name, pts, r in out]


@pytest.fixture(scope="module")
def state():
    rng = np.random.default_rng(5)
    ev = rng.integers(-127, 128, sh.DIMS).astype(np.int8)
    ev[rng.random(sh.DIMS) < 0.5] = 0
    return dict(ev=ev, before=(rng.random(sh.DIMS) < 0.2).astype(np.uint8), known=(rng.random(sh.DIMS) < 0.3).astype(np.uint8))


def stats_of(d):
    return [d[k] for k in eh.STATS]


def scan(g, pts, max_range, par=eh.DEFAULTS, inflate=(0, 0, 0), mode="continue", origin=sh.ORIGIN, lower=sh.LOWER, upper=sh.UPPER, **kw):
    return g.integrate_scan_evidence(pts, origin, lower, sh.RES, max_range, inflate=inflate, mode=mode, map_upper=upper, **par, **kw)


def check(g, st, want, what):
    for name, got in (("ev", g.evidence_grid()), ("raw", g.scan_grid()), ("map", g.get_map())):
        assert got.dtype == want[name].dtype and np.array_equal(got, want[name]), (what, name, int((got != want[name]).sum()))
    if want["known"] is None:
        with pytest.raises(solver.DirectError):
            g.known_grid()
    else:
        assert np.array_equal(g.known_grid(), want["known"]), (what, "known")
    assert stats_of(st) == want["stats"].tolist(), (what, st, want["stats"])


@pytest.mark.parametrize("mode", ("reset", "continue", "adopt"))
def test_device_equals_the_restatement(gen, cases, state, mode):
    """both inflations and both parameter sets, tracked and untracked, from a handle that holds evidence, a map and a known grid"""
    hits = 0
    for name, pts, r, touched in cases:
        for inflate in INFLATES:
            for k, par in enumerate((eh.DEFAULTS, eh.SMALL)):
                track = bool(k) ^ (inflate == INFLATES[0])
                gen.set_map(state["before"])
                gen.set_evidence(state["ev"])
                gen.set_known(state["known"])
                want = eh.restate(pts, sh.ORIGIN, r, par, inflate, mode, state["ev"], state["before"], state["known"], track, touched=touched)
                check(gen, scan(gen, pts, r, par, inflate, mode, track_known=track), want, (name, r, inflate, par, mode))
                hits += int(want["stats"][8])
    assert hits > 0 and gen.last_ms() > 0.0


def test_a_handle_that_holds_nothing(built):
    """CONTINUE without an evidence grid, a scan grid or a map starts from zeros; ADOPT without a map is refused, and so is the getter
    before the first call"""
    pts = mh.cloud_random(300)
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    with pytest.raises(solver.DirectError, match="no evidence grid"):
        g.evidence_grid()
    with pytest.raises(solver.DirectError, match="DIRECT_SCAN_ADOPT"):
        scan(g, pts, 10.0, mode="adopt")
    w1 = eh.restate(pts, sh.ORIGIN, 10.0, eh.SMALL, (2, 2, 1), "continue", track=True)
    check(g, scan(g, pts, 10.0, eh.SMALL, (2, 2, 1), track_known=True), w1, "continue on nothing")
    w2 = eh.restate(pts, sh.ORIGIN, 10.0, eh.SMALL, (2, 2, 1), "continue", w1["ev"], w1["map"], w1["known"], True)
    check(g, scan(g, pts, 10.0, eh.SMALL, (2, 2, 1), track_known=True), w2, "continue")
    assert w2["stats"][4] > w1["stats"][4] == 0      # hit = 2 < occ = 3: the returns enter the scan grid at the second scan
    g.close()


def test_parameter_refusals_behind_the_plain_ones(gen):
    """on a handle with voxels: the plain call's last refusals (ADOPT without a map is in the test above; UNSUPPORTED here) come
    before hit, miss, ev_min, ev_max, occ, reserved, in this order; a refused call leaves the handle as it was"""
    pts = mh.cloud_random(10)
    gen.set_evidence(None)
    lib = cluster._lib()

    def call(inflate=(0, 0, 0), max_range=1.5, **ev):
        e = dict(hit=0, miss=0, ev_min=1, ev_max=0, occ=0, reserved=(1, 0, 0))
        e.update(ev)
        ms = cluster.MapScan((C.c_double * 3)(*sh.LOWER), (C.c_double * 3)(*sh.UPPER), sh.RES, max_range, (C.c_double * 3)(*sh.ORIGIN),
                             (C.c_int32 * 3)(*inflate), cluster.SCAN_CONTINUE, 3, 0)
        p = cluster.MapEvidence(ms, e["hit"], e["miss"], e["ev_min"], e["ev_max"], e["occ"], (C.c_int32 * 3)(*e["reserved"]))
        st = lib.direct_cluster_map_integrate_scan_evidence(gen.h, C.addressof(p), len(pts), abi.MEM_HOST, pts.ctypes.data, None)
        return st, lib.direct_cluster_last_error().decode()

    assert call(max_range=1e6) == (abi.DIRECT_ERR_UNSUPPORTED, "max_range above 4096 voxels")
    assert call(inflate=(0, 65, 0)) == (abi.DIRECT_ERR_UNSUPPORTED, "inflate above 64 voxels")
    for kw, word in ((dict(), "hit"), (dict(hit=128), "hit"), (dict(hit=1), "miss"), (dict(hit=1, miss=128), "miss"), (dict(hit=1, miss=1), "ev_min"),
                     (dict(hit=1, miss=1, ev_min=-128), "ev_min"), (dict(hit=1, miss=1, ev_min=0), "ev_max"),
                     (dict(hit=1, miss=1, ev_min=0, ev_max=128), "ev_max"), (dict(hit=1, miss=1, ev_min=0, ev_max=5), "occ"),
                     (dict(hit=1, miss=1, ev_min=0, ev_max=5, occ=6), "occ"), (dict(hit=1, miss=1, ev_min=0, ev_max=5, occ=5), "reserved")):
        st, msg = call(**kw)
        assert st == abi.DIRECT_ERR_INVALID and msg.startswith(word + " "), (kw, msg)
    assert not gen.evidence_grid().any()             # still there, still zero


def test_the_plain_scan_is_a_special_case_on_the_device(built):
    """two handles: plain tracked scans on one, evidence scans with (1, 1, 0, 1, 1) on the other, over four scans with a set_map in
    the middle; map, scan grid, known grid and stats[0..7] are equal after every step, and so are the frontier goals at the end"""
    pts = mh.cloud_random(1000)
    lattice = sh.cloud_lattice()
    other = ph.shared_map()
    a, b = cluster.ClusterGenerator(sh.DIMS, **SMALL), cluster.ClusterGenerator(sh.DIMS, **SMALL)

    def both(cloud, r, inflate, mode):
        sa = a.integrate_scan(cloud, sh.ORIGIN, sh.LOWER, sh.RES, r, inflate=inflate, mode=mode, map_upper=sh.UPPER, track_known=True)
        sb = scan(b, cloud, r, eh.LAST_WINS, inflate, mode, track_known=True)
        assert [sa[k] for k in sh.STATS] == [sb[k] for k in sh.STATS], (sa, sb)
        assert np.array_equal(a.get_map(), b.get_map()) and np.array_equal(a.scan_grid(), b.scan_grid()) and np.array_equal(a.known_grid(), b.known_grid())
        assert np.array_equal(b.evidence_grid(), b.scan_grid().astype(np.int8))
        return sb

    both(pts[:400], 10.0, (2, 2, 1), "continue")
    st = both(pts[400:700], 10.0, (2, 2, 1), "continue")
    assert st["set"] > 0 and st["cleared"] > 0
    a.set_map(other)
    b.set_map(other)
    both(pts[700:], 1.5, (0, 0, 0), "continue")          # the changes are counted against set_map's bytes on both
    a.set_map(other)
    b.set_map(other)
    st = both(lattice, 10.0, (1, 0, 2), "adopt")
    assert st["cleared"] > 0
    fa, fb = a.frontiers(), b.frontiers()
    assert fa["stats"] == fb["stats"] and fa["stats"]["kept"] > 0
    for k in ("label", "size", "centroid", "rep"):
        assert np.array_equal(fa[k], fb[k]), k
    a.close()
    b.close()


def test_host_and_device_points_with_both_strides(gen, state):
    import torch
    pts = np.concatenate([mh.cloud_random(1000), mh.cloud_nonfinite()])
    want = None
    for stride4 in (False, True):
        for device in (False, True):
            cloud = mh.with_stride4(pts) if stride4 else pts
            gen.set_map(state["before"])
            gen.set_evidence(torch.from_numpy(state["ev"]).cuda() if device else state["ev"])
            gen.set_known(state["known"])
            st = scan(gen, torch.from_numpy(np.ascontiguousarray(cloud)).cuda() if device else cloud, 10.0, eh.SMALL, (2, 2, 1), track_known=True)
            got = (gen.evidence_grid(), gen.scan_grid(), gen.get_map(), gen.known_grid(), stats_of(st))
            if want is None:
                want = got
                w = eh.restate(pts, sh.ORIGIN, 10.0, eh.SMALL, (2, 2, 1), "continue", state["ev"], state["before"], state["known"], True)
                check(gen, st, w, "host, stride 3")
            for x, y in zip(got, want):
                assert np.array_equal(x, y), (stride4, device)


def test_a_voxel_count_that_is_no_multiple_of_16(built):
    """9 x 7 x 5 = 315 voxels with inflate (15, 15, 7): the fold's tail of 11 voxels and the cut boxes"""
    dims, lower = (9, 7, 5), np.array([0.3, -0.45, 0.15])
    upper = lower + np.array(dims) * sh.RES
    origin = lower + np.array([4.3, 3.6, 2.2]) * sh.RES
    pts = np.concatenate([mh.cloud_random(40, dims, sh.RES, lower, seed=4), mh.cloud_borders(dims, sh.RES, lower, upper)])
    rng = np.random.default_rng(1)
    ev = rng.integers(-127, 128, dims).astype(np.int8)
    before = (rng.random(dims) < 0.4).astype(np.uint8)
    kw = dict(dims=dims, lower=lower, upper=upper)
    g = cluster.ClusterGenerator(dims, **SMALL)
    for mode in ("reset", "continue", "adopt"):
        for inflate in ((0, 0, 0), (15, 15, 7)):
            g.set_map(before)
            g.set_evidence(ev)
            g.set_known(before)
            want = eh.restate(pts, origin, 1.0, eh.SMALL, inflate, mode, ev, before, before, True, **kw)
            assert want["touch"].ravel()[-11:].any()
            check(g, scan(g, pts, 1.0, eh.SMALL, inflate, mode, origin=origin, lower=lower, upper=upper, track_known=True), want, (mode, inflate))
    g.close()


def _constant(header, name):
    text = open(os.path.join(ROOT, "direct_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_a_map_on_which_the_fold_takes_a_second_trip(built):
    """kScanMaxBlocks workgroups of 256 lanes with kEvidGroup voxels each cover 4 194 304 voxels in one trip: 1024 x 257 x 16 is the
    smallest map of this shape beyond that (below 8 M voxels, so the launch is the shipped one).  Two axis-parallel rays, one of them
    through the voxels of the second trip; the expectation is NumPy alone."""
    one_trip = _constant("map_scan.h", "kScanMaxBlocks") * 256 * _constant("map_evidence.h", "kEvidGroup")
    dims = (1024, one_trip // (1024 * 16) + 1, 16)
    G = int(np.prod(dims))
    assert one_trip < G < 8 << 20 and dims[1] <= 1024
    y, z = dims[1] // 2, 8
    first_x_of_trip_2 = -(-one_trip // (dims[1] * dims[2]))
    assert first_x_of_trip_2 < 1023
    lower = np.zeros(3)
    centre = lambda x: ((np.array([x, y, z]) + 0.5) * sh.RES).astype(np.float32)
    origin = centre(1000).astype(np.float64)
    pts = np.stack([centre(1023), centre(990)])
    rng = np.random.default_rng(7)
    ev0 = rng.integers(-6, 7, dims).astype(np.int8)
    par = eh.SMALL
    want = ev0.astype(np.int32)
    line = want[:, y, z]
    line[991:1023] = np.maximum(line[991:1023] - par["miss"], par["ev_min"])      # passed: the origin's voxel once, whichever ray
    line[[990, 1023]] = np.minimum(line[[990, 1023]] + par["hit"], par["ev_max"])
    raw = (want >= par["occ"]).astype(np.uint8)
    g = cluster.ClusterGenerator(dims, max_batch=1, cluster_capacity=64, candidate_capacity=64)
    g.set_evidence(ev0)
    st = g.integrate_scan_evidence(pts, origin, lower, sh.RES, 10.0, **par)
    got = g.evidence_grid()
    assert np.array_equal(got, want.astype(np.int8)), int((got != want).sum())
    assert np.array_equal(g.scan_grid(), raw) and np.array_equal(g.get_map(), raw)
    assert stats_of(st) == [2, 0, 0, 0, int(raw.sum()), int(raw.sum()), int(raw.sum()), 0, 2, 32, int((want > 0).sum()), int((want < 0).sum())]
    assert (raw.ravel()[one_trip:] == 1).any() and (want.ravel()[one_trip:] != ev0.ravel()[one_trip:]).any()
    g.close()


def test_nothing_changed_keeps_the_field_and_the_first_flip_makes_it_stale(built):
    par = eh.SMALL
    wpts, room, wall = sh.wall_and_room()
    w = tuple(wall.T)
    both = np.concatenate([wpts, room])
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    for _ in range(4):                                       # saturated on both sides after max(ceil(5 / 2), 3) = 3 scans
        st = scan(g, both, 10.0, par)
    assert st["set"] + st["cleared"] == 0 and g.get_map()[w].all()
    ev = g.evidence_grid()
    assert (ev[w] == par["ev_max"]).all() and ev.min() == par["ev_min"]
    g.build_distance_field()
    d2 = g.distance_field()
    st = scan(g, both, 10.0, par)                            # a saturated static room scanned again
    assert st["set"] + st["cleared"] == 0 and np.array_equal(g.evidence_grid(), ev)
    assert np.array_equal(g.distance_field(), d2)            # still served
    for k in range(1, par["ev_max"] - par["occ"] + 2):       # the wall is gone: it leaves after exactly ev_max - occ + 1 scans
        st = scan(g, room, 10.0, par)
        last = k == par["ev_max"] - par["occ"] + 1
        assert (st["cleared"] == len(wall)) == last and st["set"] == 0 and g.get_map()[w].all() != last
        if not last:
            assert np.array_equal(g.distance_field(), d2)
    with pytest.raises(solver.DirectError, match="no valid distance field"):
        g.distance_field()                                   # the scan that first flips a voxel makes it stale
    g.close()


def test_the_state_rows_through_the_python_api(built):
    pts = mh.cloud_random(500)
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)

    def holds():
        out = []
        for name in ("evidence_grid", "scan_grid", "get_map", "known_grid"):
            try:
                getattr(g, name)()
                out.append(True)
            except solver.DirectError:
                out.append(False)
        return out

    assert holds() == [False, False, False, False]
    with pytest.raises(solver.DirectError, match="hit must"):
        scan(g, pts, 10.0, dict(eh.SMALL, hit=0))
    assert holds() == [False, False, False, False]           # a refused call leaves the handle as it was
    scan(g, pts, 10.0, eh.SMALL, track_known=True)
    assert holds() == [True, True, True, True]
    scan(g, pts, 10.0, eh.SMALL)                             # untracked: the known grid is dropped, as by the plain scan
    assert holds() == [True, True, True, False]
    ev = g.evidence_grid()
    g.set_map(ph.shared_map())                               # set_map keeps the evidence
    assert holds() == [True, True, True, False] and np.array_equal(g.evidence_grid(), ev)
    g.set_map_from_cloud(pts, sh.LOWER, sh.RES, 0.25, map_upper=sh.UPPER)
    assert holds() == [True, True, True, False] and np.array_equal(g.evidence_grid(), ev)
    g.integrate_scan(pts, sh.ORIGIN, sh.LOWER, sh.RES, 10.0, map_upper=sh.UPPER, track_known=True)   # a plain scan drops the evidence
    assert holds() == [False, True, True, True]
    with pytest.raises(solver.DirectError):
        g.integrate_scan(pts, sh.ORIGIN, sh.LOWER, sh.RES, -1.0, map_upper=sh.UPPER)
    rng = np.random.default_rng(3)
    mine = rng.integers(-128, 128, sh.DIMS).astype(np.int8)
    mine.ravel()[:4] = (-128, -127, 127, 0)
    raw, old = g.scan_grid(), g.get_map()
    g.set_evidence(mine)                                     # ready once drained; -128 is stored as -127; map and scan grid untouched
    assert holds() == [True, True, True, True]
    assert np.array_equal(g.evidence_grid(), np.maximum(mine, -127)) and np.array_equal(g.scan_grid(), raw) and np.array_equal(g.get_map(), old)
    g.frontiers()
    assert holds() == [True, True, True, True]               # frontier keeps it
    for occ in (3, 1, 100):                                  # set_evidence, then a scan of no points: raw == (ev >= occ)
        st = scan(g, pts[:0], 10.0, dict(eh.DEFAULTS, ev_max=127, occ=occ), track_known=True)
        want = (np.maximum(mine, -127).astype(np.int32) >= occ).astype(np.uint8)
        assert np.array_equal(g.scan_grid(), want) and np.array_equal(g.get_map(), want) and st["touched_hit"] == st["touched_pass"] == 0
        assert np.array_equal(g.evidence_grid(), np.maximum(mine, -127)) and st["raw_occupied"] == int(want.sum())
    g.set_evidence(None)
    assert not g.evidence_grid().any()
    g.close()
