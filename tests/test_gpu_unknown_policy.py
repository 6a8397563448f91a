"""The unknown policy of the cluster handle (include/direct_cluster.h, "unknown space as occupied"; kernel k_scan_close in
direct_amd/csrc/map_close.h) on the device: both scans under DIRECT_UNKNOWN_OCCUPIED against the restatement of
tests/unknown_policy_harness.py (held equal to the g++ build of map_close_math.h by tests/test_unknown_policy_restatement.py), the
open map against a second handle under DIRECT_UNKNOWN_FREE, and the planning calls on the closed map.  Grids are bytes and stats
are counts: everything is compared for equality."""
import os
import re

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import evidence_harness as eh
from tests import grid_path_harness as gh
from tests import map_cloud_harness as mh
from tests import map_scan_harness as sh
from tests import plan_check_harness as ph
from tests import unknown_policy_harness as uh

pytestmark = pytest.mark.gpu
ROOT = sh.ROOT
SMALL = dict(max_batch=4, cluster_capacity=64, candidate_capacity=64)
INFLATES = ((0, 0, 0), (2, 2, 1))
MODES = ("reset", "continue", "adopt")
NO_OPEN = "the handle has no open map"


def new_handle(policy=None, dims=sh.DIMS, **kw):
    g = cluster.ClusterGenerator(dims, **(kw or SMALL))
    if policy:
        g.set_unknown_policy(policy)
    return g


@pytest.fixture(scope="module")
def occ(built):
    g = new_handle("occupied")
    yield g
    g.close()


@pytest.fixture(scope="module")
def free(built):
    g = new_handle()
    yield g
    g.close()


@pytest.fixture(scope="module")
def cases():
    """(name, points, range, touch grid) once: n = 0, below, at and above one wave and several workgroups of the random cloud, and
    the lattice; shared and left unchanged"""
    clouds = sh.clouds()
    out = [("random_%d" % n, clouds["random"][:n], 1.5) for n in (0, 1, 63, 64, 65)]
    out += [("random_1000", clouds["random"], r) for r in sh.RANGES] + [("lattice", clouds["lattice"], 10.0)]
    return [(name, pts, r, eh.touch_grid(pts, sh.ORIGIN, r)) for name, pts, r in out]


@pytest.fixture(scope="module")
def state():
    rng = np.random.default_rng(5)
    ev = rng.integers(-127, 128, sh.DIMS).astype(np.int8)
    ev[rng.random(sh.DIMS) < 0.5] = 0
    return dict(ev=ev, before=(rng.random(sh.DIMS) < 0.2).astype(np.uint8), known=(rng.random(sh.DIMS) < 0.3).astype(np.uint8))


def plain(g, pts, r, inflate=(0, 0, 0), mode="continue", track=True, origin=sh.ORIGIN, lower=sh.LOWER, upper=sh.UPPER):
    return g.integrate_scan(pts, origin, lower, sh.RES, r, inflate=inflate, mode=mode, map_upper=upper, track_known=track)


def evidence(g, pts, r, par=eh.SMALL, inflate=(0, 0, 0), mode="continue", track=True, origin=sh.ORIGIN, lower=sh.LOWER, upper=sh.UPPER):
    return g.integrate_scan_evidence(pts, origin, lower, sh.RES, r, inflate=inflate, mode=mode, map_upper=upper, track_known=track, **par)


def scan_grid_or_none(g):
    try:
        return g.scan_grid()
    except solver.DirectError:
        return None


def check(g, st, want, what):
    """map, open map, scan grid, known grid, evidence where the scan has one, every stat and the two policy counts"""
    grids = [("map", g.get_map()), ("open", g.open_map()), ("raw", g.scan_grid()), ("known", g.known_grid())]
    if "ev" in want:
        grids.append(("ev", g.evidence_grid()))
    for name, got in grids:
        assert got.dtype == want[name].dtype and np.array_equal(got, want[name]), (what, name, int((got != want[name]).sum()))
    names = eh.STATS if "ev" in want else sh.STATS
    assert [st[k] for k in names] == want["stats"].tolist(), (what, st, want["stats"])
    assert g.unknown_policy() == dict(policy="occupied", closed=want["closed"], open_ones=want["open_ones"]), what


@pytest.mark.parametrize("mode", MODES)
def test_device_equals_the_restatement(occ, cases, state, mode):
    """1.  both scans, both inflations, from a handle seeded by set_map / set_known / set_evidence"""
    closed = 0
    for name, pts, r, touched in cases:
        for k, inflate in enumerate(INFLATES):
            occ.set_map(state["before"])
            occ.set_known(state["known"])
            raw0 = scan_grid_or_none(occ)                            # what the scan before this one left
            want = uh.restate_plain(pts, sh.ORIGIN, r, inflate, mode, raw0, state["before"], state["known"], touched=touched)
            check(occ, plain(occ, pts, r, inflate, mode), want, ("plain", name, r, inflate, mode))
            occ.set_map(state["before"])
            occ.set_known(state["known"])
            occ.set_evidence(state["ev"])
            par = (eh.DEFAULTS, eh.SMALL)[k]
            want = uh.restate_evidence(pts, sh.ORIGIN, r, par, inflate, mode, state["ev"], state["before"], state["known"], touched=touched)
            check(occ, evidence(occ, pts, r, par, inflate, mode), want, ("evidence", name, r, inflate, mode))
            closed += want["closed"]
    assert closed > 0 and occ.last_ms() > 0.0


def sequence(pts, lattice):
    """(kind, cloud, range, inflate, mode): plain and evidence scans, every mode, both inflations"""
    return (("plain", pts[:400], 10.0, (2, 2, 1), "continue"), ("plain", pts[400:700], 1.5, (2, 2, 1), "continue"),
            ("evidence", pts[700:], 10.0, (0, 0, 0), "continue"), ("evidence", lattice, 1.5, (2, 2, 1), "continue"),
            ("plain", lattice, 10.0, (1, 0, 2), "reset"), ("evidence", pts[:300], 10.0, (2, 2, 1), "reset"))


@pytest.fixture(scope="module")
def pair(built):
    """two handles after the same scan sequence, the first under the policy, the second not; compared after every step"""
    pts, lattice = mh.cloud_random(1000), sh.cloud_lattice()
    a, b = new_handle("occupied"), new_handle()
    for kind, cloud, r, inflate, mode in sequence(pts, lattice):
        sa, sb = ((plain(g, cloud, r, inflate, mode) if kind == "plain" else evidence(g, cloud, r, eh.LAST_WINS, inflate, mode)) for g in (a, b))
        assert np.array_equal(a.open_map(), b.get_map()), (kind, mode)                      # 2. the open map IS the map under FREE
        assert np.array_equal(a.scan_grid(), b.scan_grid()) and np.array_equal(a.known_grid(), b.known_grid())
        if kind == "evidence":
            assert np.array_equal(a.evidence_grid(), b.evidence_grid())
        kn = a.known_grid() != 0
        assert np.array_equal(a.get_map(), (a.open_map() | ~kn).astype(np.uint8))
        assert [sa[k] for k in sh.STATS[:5]] == [sb[k] for k in sh.STATS[:5]]
        assert a.unknown_policy()["open_ones"] == sb["occupied"] and sa["occupied"] == sb["occupied"] + a.unknown_policy()["closed"]
        fa, fb = a.frontiers(), b.frontiers()                                               # 6. the frontier is the same on both
        assert fa["stats"] == fb["stats"]
        for k in ("label", "size", "centroid", "rep"):
            assert np.array_equal(fa[k], fb[k]), (k, kind, mode)
    yield a, b
    a.close()
    b.close()


def test_open_map_pinned_against_a_second_handle(pair):
    """2.  every step's comparison is in the fixture; here what is left: the second handle has no open map and reports FREE"""
    a, b = pair
    assert a.unknown_policy()["policy"] == "occupied" and b.unknown_policy() == dict(policy="free", closed=0, open_ones=0)
    with pytest.raises(solver.DirectError, match=NO_OPEN):
        b.open_map()
    assert a.frontiers()["stats"]["kept"] > 0 and a.unknown_policy()["closed"] > 0


def test_free_is_untouched(built, state):
    """3.  occupied, then free, then scans: every grid and stat equals a fresh handle's, and there is no open map"""
    pts, lattice = mh.cloud_random(1000), sh.cloud_lattice()
    a, b = new_handle(), new_handle()
    a.set_unknown_policy("occupied")
    a.set_unknown_policy("free")
    for g in (a, b):
        g.set_map(state["before"])
    for kind, cloud, r, inflate, mode in sequence(pts, lattice) + (("plain", pts, 10.0, (2, 2, 1), "adopt"),):
        for track in (True, False):
            sa, sb = ((plain(g, cloud, r, inflate, mode, track) if kind == "plain" else evidence(g, cloud, r, eh.SMALL, inflate, mode, track))
                      for g in (a, b))
            assert sa == sb, (kind, mode, track)
            for name in ("get_map", "scan_grid") + (("known_grid",) if track else ()) + (("evidence_grid",) if kind == "evidence" else ()):
                assert np.array_equal(getattr(a, name)(), getattr(b, name)()), (name, kind, mode, track)
            with pytest.raises(solver.DirectError, match=NO_OPEN):
                a.open_map()
            assert a.unknown_policy() == dict(policy="free", closed=0, open_ones=0)
    a.close()
    b.close()


def test_the_planners_stay_inside_known_space(built, tmp_path):
    """4.  the reason for the feature: an L-shaped known region on an empty map, start and goal at its far ends.  Under FREE the
    cheapest path cuts through unobserved space (checked on the CPU first); under OCCUPIED every planning call stays inside."""
    sc = uh.l_scene()
    known, start, goal = sc["known"], np.array([sc["start"]], np.int32), np.array([sc["goal"]], np.int32)
    dj = gh.build(tmp_path)
    empty = np.zeros(sh.DIMS, np.uint8)
    loose = uh.dijkstra(dj, empty, start, goal)
    assert loose["rtn"][0] == gh.OK and any(known[tuple(v)] == 0 for v in loose["paths"][0])
    g = new_handle("occupied")
    g.set_known(known)
    st = plain(g, mh.cloud_random(0), 10.0)                       # a CONTINUE tracked scan of no points derives the map
    closed = (known == 0).astype(np.uint8)
    assert np.array_equal(g.get_map(), closed) and not g.open_map().any() and st["occupied"] == st["set"] == int(closed.sum())
    tight = uh.dijkstra(dj, closed, start, goal)
    assert tight["rtn"][0] == gh.OK and tight["path_cost"][0] > loose["path_cost"][0]
    g.build_distance_field()
    assert (g.distance_field()[known == 0] == 0).all() and (g.distance_field()[known == 1] > 0).all()
    paths = dict(pair=g.grid_paths(start, goal), clear=g.grid_paths_clear(start, goal), fan=g.grid_paths_fan(start, goal))
    for name, r in paths.items():
        assert r["rtn"][0] == cluster.GRID_PATH_OK and r["path_cost"][0] == tight["path_cost"][0], name
        assert all(known[tuple(v)] == 1 for v in r["paths"][0]) and len(r["paths"][0]) == r["path_len"][0] > 12, name
    path = paths["pair"]["paths"][0]
    xyz = np.zeros((1, 128, 3), np.int32)
    xyz[0, :len(path)] = path
    cor = g.cube_corridors(xyz, np.array([len(path)], np.int32), sh.LOWER, sh.RES, seg_capacity=64)
    assert cor["rtn"][0] == cluster.CUBE_CORRIDOR_OK and cor["n_seg"][0] >= 2
    for lo_hi in cor["cube_idx"][0, :cor["n_seg"][0]]:
        lo, hi = lo_hi[:3], lo_hi[3:]
        assert known[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1].all(), lo_hi
    g.build_free_components()
    rtn, _, size = g.reachable(np.concatenate([start, start]), np.array([sc["goal"], sc["island_goal"]], np.int32))
    assert rtn.tolist() == [cluster.GRID_PATH_OK, cluster.GRID_PATH_NO_PATH] and size[1] == 6 * 6 * 3   # only unknown space connects the island
    centre = lambda v: np.asarray(sh.LOWER) + (np.asarray(v) + 0.5) * sh.RES
    plan = ph.pick(ph.pack([[(ph._line(centre(sc["start"]), centre(sc["goal"])), 1.0)]], 1), "bez")
    verdict = g.check_plans(plan["n_seg"], plan["T"], sh.LOWER, sh.RES, bez=plan["bez"])
    assert verdict["status"][0] == 0 and verdict["verdict"][0] == 1                          # the straight plan is not clear
    g.close()


def test_view_gain_reads_the_open_map(pair):
    """5.  every output equals the FREE handle's, with unknown voxels counted - which rays stopped by the closed map could not"""
    a, b = pair
    reps = a.frontiers()["rep"]
    dirs = cluster.view_directions(16, 5, -0.6, 0.6)
    va, vb = a.view_gain(reps, dirs, 8.0), b.view_gain(reps, dirs, 8.0)
    for k in ("code", "gain", "seen", "ends"):
        assert np.array_equal(va[k], vb[k]), k
    assert len(reps) > 0 and (va["code"] == cluster.VIEW_OK).all() and (va["gain"] > 0).any()


def test_frontiers_are_equal_under_both_policies(occ, free, cases, state):
    """6.  on the scenes of test 1: both handles seeded alike, every mode"""
    for name, pts, r, _ in cases[-3:]:
        for mode in MODES:
            for g in (occ, free):
                g.set_map(state["before"])
                g.set_known(state["known"])
                plain(g, pts, r, (2, 2, 1), mode)
            fa, fb = occ.frontiers(min_d2=0), free.frontiers(min_d2=0)
            assert fa["stats"] == fb["stats"], (name, mode)
            # not vacuous where the scan grid starts from what was carved; ADOPT of the seeded 20 % map dilated by (2, 2, 1) leaves
            # few known free voxels (the restatement counts 4, 17 and, for the lattice, 0 frontier voxels)
            assert mode == "adopt" or fa["stats"]["frontier"] > 100, (name, mode, fa["stats"])
            for k in ("label", "size", "centroid", "rep"):
                assert np.array_equal(fa[k], fb[k]), (name, mode, k)
            assert (occ.get_map()[tuple(fa["rep"].T)] == 0).all()              # every representative stays a legal goal


def test_a_scan_that_teaches_nothing_keeps_the_field(built):
    """7.  the same scan twice: set + cleared == 0 and the field serves; one new voxel observed and it is stale"""
    wpts, room, _ = sh.wall_and_room()
    both = np.concatenate([wpts, room])
    g = new_handle("occupied")
    first = plain(g, both, 10.0)
    assert first["set"] > 0
    g.build_distance_field()
    again = plain(g, both, 10.0)
    assert again["set"] + again["cleared"] == 0 and again["occupied"] == first["occupied"]
    known = g.known_grid()
    enterable = np.argwhere(g.get_map() == 0)
    s, t = enterable[0][None], enterable[-1][None]
    r = g.grid_paths_clear(s, t, min_d2=2)                                   # with a floor: not refused
    assert r["rtn"][0] in (cluster.GRID_PATH_OK, cluster.GRID_PATH_NO_PATH, cluster.GRID_PATH_BAD_ENDPOINT)
    unknown = np.argwhere(known == 0)
    assert len(unknown) > 0
    # a ray from the origin through the centre of the unknown voxel nearest to it, ending far beyond the range: it is truncated,
    # marks nothing and carves that voxel, which leaves the map
    v = unknown[np.argmin(((unknown - np.array([22, 16, 6])) ** 2).sum(axis=1))]
    p = (sh.ORIGIN + 100.0 * (sh.LOWER + (v + 0.5) * sh.RES - sh.ORIGIN)).astype(np.float32)[None]
    third = plain(g, p, 10.0)
    assert third["truncated"] == 1 and third["cleared"] >= 1 and third["set"] == 0
    assert g.known_grid()[tuple(v)] == 1 and g.get_map()[tuple(v)] == 0
    with pytest.raises(solver.DirectError, match="no valid distance field"):
        g.grid_paths_clear(s, t, min_d2=2)
    g.close()


def test_point_order_does_not_matter(occ, state):
    """8a.  shuffled points give identical bytes"""
    pts = np.concatenate([mh.cloud_random(1000), sh.cloud_lattice()])
    shuffled = pts[np.random.default_rng(3).permutation(len(pts))]
    got = []
    for cloud in (pts, shuffled):
        occ.set_map(state["before"])
        occ.set_known(state["known"])
        st = plain(occ, cloud, 10.0, (2, 2, 1), "reset")
        got.append((occ.get_map(), occ.open_map(), occ.scan_grid(), occ.known_grid(), st, occ.unknown_policy()))
    for x, y in zip(*got):
        assert x == y if isinstance(x, dict) else np.array_equal(x, y)


def _constant(header, name):
    text = open(os.path.join(ROOT, "direct_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_a_map_on_which_the_close_pass_takes_a_second_trip(built):
    """8b.  kScanMaxBlocks workgroups of 256 lanes with 16 voxels each cover 4 194 304 voxels in one trip: 1024 x 257 x 16 is the
    smallest map of this shape beyond that.  Two axis-parallel rays, one through the voxels of the second trip, over a seeded known
    grid; the expectation is NumPy alone."""
    one_trip = _constant("map_scan.h", "kScanMaxBlocks") * 256 * _constant("map_close_math.h", "kGroup")
    dims = (1024, one_trip // (1024 * 16) + 1, 16)
    G = int(np.prod(dims))
    assert one_trip < G < 8 << 20 and dims[1] <= 1024
    y, z = dims[1] // 2, 8
    centre = lambda x: ((np.array([x, y, z]) + 0.5) * sh.RES).astype(np.float32)
    origin = centre(1000).astype(np.float64)
    pts = np.stack([centre(1023), centre(990)])
    known = (np.random.default_rng(7).random(dims) < 0.5).astype(np.uint8)
    raw = np.zeros(dims, np.uint8)
    raw[[990, 1023], y, z] = 1
    want_known = known.copy()
    want_known[990:1024, y, z] = 1
    want = raw | (want_known == 0).astype(np.uint8)
    g = new_handle("occupied", dims, max_batch=1, cluster_capacity=64, candidate_capacity=64)
    g.set_known(known)
    st = g.integrate_scan(pts, origin, np.zeros(3), sh.RES, 10.0, track_known=True)
    got = g.get_map()
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(g.open_map(), raw) and np.array_equal(g.scan_grid(), raw) and np.array_equal(g.known_grid(), want_known)
    ones = int(want.sum())
    assert [st[k] for k in sh.STATS] == [2, 0, 0, 0, 2, ones, ones, 0]
    assert g.unknown_policy() == dict(policy="occupied", closed=ones - 2, open_ones=2)
    tail = want.ravel()[one_trip:]
    assert (tail == 1).any() and (tail == 0).any() and raw.ravel()[one_trip:].any()
    g.close()


def test_refusals_on_a_real_handle(occ, state):
    """9.  an untracked scan under the policy is refused behind every refusal the calls have, and the handle is left as it was;
    ADOPT adopts the open map, so that unknown voxels do not become returns"""
    pts = mh.cloud_random(300)
    occ.set_map(state["before"])
    occ.set_known(state["known"])
    occ.set_evidence(state["ev"])
    evidence(occ, pts, 10.0, eh.SMALL, (2, 2, 1))
    held = lambda: [occ.get_map(), occ.open_map(), occ.scan_grid(), occ.known_grid(), occ.evidence_grid(), occ.unknown_policy()]
    before = held()
    for call in (lambda **kw: plain(occ, pts, track=False, **kw), lambda **kw: evidence(occ, pts, track=False, **kw)):
        with pytest.raises(solver.DirectError, match="DIRECT_SCAN_TRACK_KNOWN") as e:
            call(r=10.0)
        assert e.value.status == abi.DIRECT_ERR_INVALID
        with pytest.raises(solver.DirectError, match="max_range above 4096 voxels"):     # the last refusal of today comes first
            call(r=1e6)
        with pytest.raises(solver.DirectError, match="inflate above 64 voxels"):
            call(r=10.0, inflate=(0, 65, 0))
    with pytest.raises(solver.DirectError, match="hit must"):
        evidence(occ, pts, 10.0, dict(eh.SMALL, hit=0), track=False)
    for x, y in zip(held(), before):
        assert x == y if isinstance(x, dict) else np.array_equal(x, y)
    closed_map, opened, _, known, ev, _ = before
    for kind in ("plain", "evidence"):
        if kind == "plain":
            want = uh.restate_plain(pts[:50], sh.ORIGIN, 1.5, (2, 2, 1), "adopt", None, closed_map, known, opened)
            st = plain(occ, pts[:50], 1.5, (2, 2, 1), "adopt")
        else:
            want = uh.restate_evidence(pts[:50], sh.ORIGIN, 1.5, eh.SMALL, (2, 2, 1), "adopt", ev, closed_map, known, opened)
            st = evidence(occ, pts[:50], 1.5, eh.SMALL, (2, 2, 1), "adopt")
        check(occ, st, want, ("adopt", kind))
        unseen = (want["known"] == 0)
        assert unseen.any() and not occ.scan_grid()[unseen & (opened == 0)].any() and closed_map[unseen].all()
        closed_map, opened, known = occ.get_map(), occ.open_map(), occ.known_grid()


def test_the_state_rows_through_the_python_api(built):
    """10.  the open map's column of DESIGN.md 6.22; the rows that need a device error are covered on the CPU"""
    pts = mh.cloud_random(500)
    g = new_handle()

    def holds():
        out = []
        for name in ("open_map", "get_map", "scan_grid", "known_grid", "evidence_grid"):
            try:
                getattr(g, name)()
                out.append(True)
            except solver.DirectError:
                out.append(False)
        return out

    assert holds() == [False] * 5 and g.unknown_policy() == dict(policy="free", closed=0, open_ones=0)
    g.set_unknown_policy("occupied")                              # touches no grid, raises no map event
    assert holds() == [False] * 5 and g.unknown_policy()["policy"] == "occupied"
    with pytest.raises(ValueError):
        g.set_unknown_policy("closed")
    with pytest.raises(solver.DirectError, match="DIRECT_SCAN_TRACK_KNOWN"):
        plain(g, pts, 10.0, track=False)                          # a refused scan leaves the handle as it was
    assert holds() == [False] * 5
    plain(g, pts, 10.0)                                           # a successful scan under OCCUPIED: ready
    assert holds() == [True, True, True, True, False] and g.unknown_policy()["closed"] > 0
    g.build_distance_field()
    g.build_free_components()
    g.frontiers()
    g.set_known(g.known_grid())
    g.set_evidence(None)
    assert holds() == [True] * 5                                  # every other row keeps it
    g.set_unknown_policy("free")                                  # ... and so does the policy setter: the next scan decides
    opened = g.open_map()
    assert holds() == [True] * 5 and g.unknown_policy() == dict(policy="free", closed=g.unknown_policy()["closed"], open_ones=int(opened.sum()))
    plain(g, pts, 10.0)                                           # a scan under FREE: lost, and the map is the open map again
    assert holds() == [False, True, True, True, False] and np.array_equal(g.get_map(), opened)
    assert g.unknown_policy() == dict(policy="free", closed=0, open_ones=0)
    g.set_unknown_policy("occupied")
    evidence(g, pts, 10.0)
    assert holds() == [True] * 5
    other = ph.shared_map()
    g.set_map(other)                                              # set_map writes the caller's bytes verbatim and drops the open map
    assert holds() == [False, True, True, True, True] and np.array_equal(g.get_map(), other)
    evidence(g, pts, 10.0)
    assert holds() == [True] * 5
    g.set_map_from_cloud(pts, sh.LOWER, sh.RES, 0.25, map_upper=sh.UPPER)
    assert holds() == [False, True, True, True, True]
    with pytest.raises(solver.DirectError, match="max_range must be"):
        plain(g, pts, -1.0)
    assert holds() == [False, True, True, True, True]
    g.close()
