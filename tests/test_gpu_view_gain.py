"""Visible unknown volume per candidate viewpoint on the device (include/direct_cluster.h, "visible unknown volume per candidate
viewpoint"; kernel in direct_amd/csrc/view_gain.h) against the restatement in Python floats of tests/view_gain_harness.py, which
tests/test_view_gain_restatement.py holds equal to the g++ build of the same header.  The outputs are counts: everything is
compared for equality."""
import os
import struct
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, solver
from tests import map_scan_harness as sh
from tests import view_gain_harness as vh

pytestmark = pytest.mark.gpu
ROOT = sh.ROOT
SMALL = dict(max_batch=4, cluster_capacity=64, candidate_capacity=64)
ORIGIN_VOXEL = (22, 16, 6)
POOL = np.concatenate([vh.dirs_sign(), vh.dirs_degenerate(), vh.dirs_random(2100)])


def refused(word, call, status=abi.DIRECT_ERR_INVALID):
    with pytest.raises(solver.DirectError) as e:
        call()
    assert e.value.status == status and word in str(e.value), str(e.value)


def handle_of(scene):
    grid, known = vh.scenes()[scene]
    g = cluster.ClusterGenerator(grid.shape, **SMALL)
    g.set_map(grid)
    g.set_known(known)
    return g, grid, known


@pytest.fixture(scope="module")
def gen(built):
    g, grid, known = handle_of("random")
    yield g, grid, known
    g.close()


def test_ray_counts_around_a_wave_and_a_workgroup(gen):
    """n_dirs below, at and above one wave, a quarter of the workgroup's 1024 lanes, all of them (a lane's second ray) and twice that,
    at range 10 (R = 12); the border, corner, occupied and outside candidates of vh.candidates among them"""
    g, grid, known = gen
    cand = vh.candidates(grid)
    for n_dirs in (1, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 2049):
        want = vh.restate(grid, known, cand, POOL[:n_dirs], 10.0)
        vh.assert_same(g.view_gain(cand, POOL[:n_dirs], 10.0), want, n_dirs)
    codes = set(want["code"].tolist())
    assert codes == {vh.OK, vh.OUTSIDE, vh.OCCUPIED} and want["ends"][:, vh.SKIPPED].any() and want["ends"][:, vh.BLOCKED].any()
    assert g.last_ms() > 0.0


def test_candidate_counts(built):
    """one, two and 300 workgroups on the scanned scene"""
    g, grid, known = handle_of("wall_and_room")
    cand = vh.candidates(grid, n_free=300)[:300]
    dirs = POOL[:48]
    want = vh.restate(grid, known, cand, dirs, 10.0)
    free = np.flatnonzero(want["code"] == vh.OK)
    assert len(cand) == 300 and len(free) > 250 and (want["gain"] > 0).any() and (want["gain"][free] < want["seen"][free]).any()
    for pick in (free[:1], free[5:7], np.arange(300)):
        got = g.view_gain(cand[pick], dirs, 10.0)
        vh.assert_same(got, {k: want[k][pick] for k in vh.KEYS}, len(pick))
    g.close()


@pytest.mark.parametrize("scene", sorted(vh.scenes()))
def test_scenes_in_host_and_device_memory(built, scene):
    import torch
    g, grid, known = handle_of(scene)
    cand, dirs = vh.candidates(grid), POOL[:150]
    want = vh.restate(grid, known, cand, dirs, 6.5)
    for dev_in in (False, True):
        for mem in ("host", "device"):
            v, d = (torch.from_numpy(cand).to("cuda:0"), torch.from_numpy(dirs).to("cuda:0")) if dev_in else (cand, dirs)
            got = g.view_gain(v, d, 6.5, mem=mem)
            assert all(isinstance(got[k], np.ndarray) == (mem == "host") for k in vh.KEYS)
            vh.assert_same(got, want, (scene, dev_in, mem))
    if scene == "empty_unknown":
        assert np.array_equal(want["gain"], want["seen"])
    if scene == "empty_known":
        assert not want["gain"].any() and want["seen"].any()
    g.close()


def test_the_largest_box_and_the_first_unsupported_range(gen):
    """range_vox = 48.5 is R = 50: 128 788 bytes of LDS, one workgroup on a CU, on a map smaller than its box; 49.0 is refused"""
    g, grid, known = gen
    cand, dirs = vh.candidates(grid), POOL[:257]
    assert vh.box_half(48.5) == vh.MAX_R
    want = vh.restate(grid, known, cand, dirs, 48.5)
    vh.assert_same(g.view_gain(cand, dirs, 48.5), want)
    assert want["ends"][:, vh.LEFT].any() and not want["ends"][:, vh.RANGE].any()
    empty = np.zeros_like(grid)
    g.set_map(empty)                        # without obstacles every ray of a 24 x 20 x 12 map runs to the border
    long = vh.restate(empty, known, cand, dirs, 48.5)
    vh.assert_same(g.view_gain(cand, dirs, 48.5), long)
    assert long["seen"].max() > want["seen"].max()
    refused("range_vox", lambda: g.view_gain(cand, dirs, 49.0), abi.DIRECT_ERR_UNSUPPORTED)
    refused("n_dirs above", lambda: g.view_gain(cand, np.ones((65537, 3), np.float32), 10.0), abi.DIRECT_ERR_UNSUPPORTED)
    g.set_map(grid)
    vh.assert_same(g.view_gain(cand, dirs, 48.5), want)


def test_direction_sets(gen):
    g, grid, known = gen
    cand = vh.candidates(grid, n_free=20)
    sets_dirs = np.stack([vh.dirs_random(65, seed=s) for s in (1, 2, 3)] + [POOL[:65]])
    sets = np.array([(c % 7) - 1 for c in range(len(cand))], np.int32)       # -1, 4 and 5 are outside [0, 4)
    want = vh.restate(grid, known, cand, sets_dirs, 7.25, sets)
    assert (want["code"] == vh.BAD_SET).sum() >= 3 and {int(s) for s, c in zip(sets, want["code"]) if c == vh.OK} == {0, 1, 2, 3}
    for mem in ("host", "device"):
        vh.assert_same(g.view_gain(cand, sets_dirs, 7.25, sets=sets, mem=mem), want, mem)
    # set == NULL: every candidate uses set 0, whatever else the call holds
    vh.assert_same(g.view_gain(cand, sets_dirs, 7.25), vh.restate(grid, known, cand, sets_dirs[0], 7.25))
    vh.assert_same(g.view_gain(cand, sets_dirs[0], 7.25), vh.restate(grid, known, cand, sets_dirs[0], 7.25))
    # the C call with outputs left out: the others do not move
    lib, n = cluster._lib(), len(cand)
    import ctypes as C
    for keep in vh.KEYS:
        out = {k: np.full((n, 4) if k == "ends" else n, -7, np.int32) for k in vh.KEYS}
        par = cluster.ViewGainIn(7.25, n, 65, 4, abi.MEM_HOST, abi.MEM_HOST)
        io = cluster.ViewGainIO(cand.ctypes.data, sets.ctypes.data, sets_dirs.ctypes.data,
                                *[out[k].ctypes.data if k == keep else None for k in vh.KEYS])
        assert lib.direct_cluster_view_gain_batch(g.h, C.addressof(par), C.addressof(io)) == abi.DIRECT_OK
        assert np.array_equal(out[keep], want[keep]) and all((out[k] == -7).all() for k in vh.KEYS if k != keep)
    empty = g.view_gain(np.zeros((0, 3), np.int32), sets_dirs, 7.25)
    assert all(len(empty[k]) == 0 for k in vh.KEYS)


def test_two_calls_in_a_row_and_what_is_resident_around_them(gen):
    """the box and the counters are cleared per candidate; the call changes nothing the handle holds"""
    g, grid, known = gen
    g.build_free_components()
    label, size = (a.tobytes() for a in g.free_components())
    free = np.argwhere(grid == 0).astype(np.int32)
    ends = free[np.random.default_rng(4).choice(len(free), 16, replace=False)]
    reach = [np.asarray(v).tobytes() for v in g.reachable(ends[:8], ends[8:])]
    cand = np.concatenate([vh.candidates(grid, n_free=30)] * 2)               # every candidate twice: 2 x n workgroups reuse boxes
    first = g.view_gain(cand, POOL[:300], 10.0)
    g.view_gain(cand[::-1], POOL[:77], 3.5)                                   # another box size and ray count in between
    second = g.view_gain(cand, POOL[:300], 10.0)
    for k in vh.KEYS:
        assert first[k].tobytes() == second[k].tobytes(), k
        assert np.array_equal(first[k][:len(cand) // 2], first[k][len(cand) // 2:]), k
    vh.assert_same(first, vh.restate(grid, known, cand, POOL[:300], 10.0))
    assert [a.tobytes() for a in g.free_components()] == [label, size]
    assert [np.asarray(v).tobytes() for v in g.reachable(ends[:8], ends[8:])] == reach
    assert np.array_equal(g.known_grid(), known) and np.array_equal(g.get_map(), grid)


def test_the_ideal_scan_identity_on_the_device(built):
    """a tracked scan of the points centre + 64 * dir on the empty dyadic grid knows exactly the voxels the call sees from there"""
    D = vh.DYADIC
    dirs = vh.dirs_dyadic()
    pts, centre = vh.dyadic_cloud(dirs)
    g = cluster.ClusterGenerator(D["dims"], **SMALL)
    for max_range in vh.DYADIC_RANGES:
        g.integrate_scan(pts, centre, D["lower"], D["res"], max_range, mode="reset", map_upper=D["upper"], track_known=True)
        scanned = g.known_grid()
        assert not g.get_map().any()                                          # every return lies outside the map: nothing is marked
        g.set_known(None)
        got = g.view_gain([D["v0"]], dirs, max_range / D["res"])
        assert got["code"][0] == vh.OK and got["seen"][0] == got["gain"][0] == int(scanned.sum()) > 100, (max_range, got)
        count_only = g.view_gain([D["v0"]], dirs, max_range / D["res"], mem="device")
        assert int(count_only["gain"][0]) == int(scanned.sum())
        g.set_known(scanned)                                                  # after the scan nothing is left to gain from there
        after = g.view_gain([D["v0"]], dirs, max_range / D["res"])
        assert after["gain"][0] == 0 and after["seen"][0] == got["seen"][0] and np.array_equal(after["ends"], got["ends"])
        want = vh.restate(np.zeros(D["dims"], np.uint8), scanned, [D["v0"]], dirs, max_range / D["res"])
        vh.assert_same(after, want)
        seen = np.zeros(D["dims"], np.uint8)
        seen[tuple(np.array(sorted(want["visited"][0])).T)] = 1
        assert np.array_equal(seen, scanned)
    g.close()


# ---- the chain, once ----------------------------------------------------------------------------------------------------------
def test_scan_frontiers_view_gain_reachable_fan(built):
    wpts, room, _ = sh.wall_and_room()
    g = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    scan = lambda pts: g.integrate_scan(pts, sh.ORIGIN, sh.LOWER, sh.RES, 10.0, map_upper=sh.UPPER, track_known=True)
    scan(wpts)
    scan(room)
    f = g.frontiers(min_size=3, mem="device")
    rep = f["rep"]
    assert len(rep) > 0 and rep.is_cuda
    dirs = cluster.view_directions(24, 8, -0.6, 0.6)
    score = g.view_gain(rep, dirs, 12.0)                                      # device voxels, host directions, host outputs
    rep_host = rep.cpu().numpy()
    grid, known = g.get_map(), g.known_grid()
    vh.assert_same(score, vh.restate(grid, known, rep_host, dirs, 12.0))
    assert (score["code"] == vh.OK).all() and (score["gain"] > 0).any()       # a representative is known and enterable
    assert (score["ends"].sum(axis=1) == len(dirs)).all()
    g.build_free_components()
    rtn, _, _ = g.reachable(np.tile(np.array(ORIGIN_VOXEL, np.int32), (len(rep_host), 1)), rep_host)
    ok = rtn == cluster.GRID_PATH_OK
    assert ok.any()
    best = int(np.flatnonzero(ok)[np.argmax(score["gain"][ok])])
    out = g.grid_paths_fan(np.array([ORIGIN_VOXEL], np.int32), rep_host[best:best + 1])
    assert out["rtn"][0] == cluster.GRID_PATH_OK
    assert np.array_equal(out["paths"][0][0], ORIGIN_VOXEL) and np.array_equal(out["paths"][0][-1], rep_host[best])
    g.close()


def test_cpp_mirror_against_the_python_call(gen, tmp_path):
    """polyhedronGenerator::viewGain (direct_amd/host/poly_utils.hpp) gives the binding's arrays (tests/cpp/test_view_gain_gen.cpp)"""
    g, grid, known = gen
    cand = vh.candidates(grid)
    sets_dirs = np.stack([POOL[:40], vh.dirs_random(40, seed=21)])
    sets = np.array([c % 3 for c in range(len(cand))], np.int32)
    fin, exe = str(tmp_path / "in.bin"), str(tmp_path / "gen")
    calls = ((10.0, True), (48.5, False), (0.4, True))
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", *grid.shape) + grid.tobytes() + known.tobytes())
        f.write(struct.pack("<3i", len(cand), 2, 40) + cand.tobytes() + sets.tobytes() + sets_dirs.tobytes())
        f.write(struct.pack("<i", len(calls)))
        for r, with_sets in calls:
            got = g.view_gain(cand, sets_dirs, r, sets=sets if with_sets else None)
            f.write(struct.pack("<di", r, int(with_sets)) + b"".join(np.ascontiguousarray(got[k], np.int32).tobytes() for k in vh.KEYS))
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests/cpp/test_view_gain_gen.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "direct_amd/lib"), "-ldirect_ddp",
                           "-Wl,-rpath," + os.path.join(ROOT, "direct_amd/lib") + ":/opt/rocm/lib"])
    out = subprocess.run([exe, fin], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- refusals on a live handle --------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle(built):
    grid, known = vh.scenes()["random"]
    cand, dirs = vh.candidates(grid), POOL[:30]
    g = cluster.ClusterGenerator(grid.shape, **SMALL)
    call = lambda **kw: g.view_gain(cand, dirs, kw.pop("range_vox", 5.0), **kw)
    refused("no map", call)
    g.set_known(known)
    refused("no map", call)                                                   # a known grid alone is not enough
    g.set_map(grid)
    want = vh.restate(grid, known, cand, dirs, 5.0)
    vh.assert_same(call(), want)
    for bad in (lambda: call(range_vox=0.0), lambda: call(range_vox=float("nan")), lambda: call(range_vox=-2.0)):
        refused("range_vox must be finite and positive", bad)
    refused("range_vox", lambda: call(range_vox=49.0), abi.DIRECT_ERR_UNSUPPORTED)
    assert np.array_equal(g.known_grid(), known) and np.array_equal(g.get_map(), grid)
    vh.assert_same(call(), want)                                              # a refused call leaves the handle as it was
    pts = sh.mh.cloud_random(200)
    # an untracked scan drops the known grid (this map is not the scan's size: use a handle of the scan's dims for it)
    s = cluster.ClusterGenerator(sh.DIMS, **SMALL)
    scan = lambda track: s.integrate_scan(pts, sh.ORIGIN, sh.LOWER, sh.RES, 1.5, map_upper=sh.UPPER, track_known=track)
    scan(True)
    origin = np.array([ORIGIN_VOXEL], np.int32)
    seen = s.view_gain(origin, dirs, 5.0)
    assert seen["code"][0] == vh.OK and seen["seen"][0] > 1
    scan(False)
    refused("no known grid", lambda: s.view_gain(origin, dirs, 5.0))
    assert s.get_map().shape == sh.DIMS
    scan(True)
    vh.assert_same(s.view_gain(origin, dirs, 5.0), vh.restate(s.get_map(), s.known_grid(), origin, dirs, 5.0))
    s.close()
    g.close()
