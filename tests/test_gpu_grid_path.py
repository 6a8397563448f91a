"""direct_cluster_grid_path_batch (include/direct_cluster.h, "grid paths"; kernels in direct_amd/csrc/grid_path.h) on the device,
through the C-ABI, against the g++ build of the same arithmetic (tests/grid_path_harness.py, itself checked against an
independent Dijkstra by tests/test_grid_path_restatement.py): paths, lengths, costs and codes bit for bit, the field where the
contract calls it exact, every return code, launch-shape independence, device-memory outputs, the handle's resident clusters
left alone, and the chain into the corridor generator."""
import os
import struct
import subprocess

import numpy as np
import pytest

from direct_amd import abi, cluster, problems
from tests import grid_path_harness as gh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return gh.build(tmp_path_factory.mktemp("grid_path_gpu"))


@pytest.fixture(scope="module")
def big(built):
    grid = gh.big_map()
    starts, goals = gh.big_queries(grid, 64)
    gen = cluster.ClusterGenerator(grid.shape, max_batch=64, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
    yield grid, starts, goals, gen
    gen.close()


def same_paths(dev, ref, q, qr=None):
    qr = q if qr is None else qr
    assert dev["rtn"][q] == ref["rtn"][qr], (q, dev["rtn"][q], ref["rtn"][qr])
    assert dev["path_len"][q] == ref["path_len"][qr]
    assert bits(dev["path_cost"][q]) == bits(ref["path_cost"][qr]) or (np.isnan(dev["path_cost"][q]) and np.isnan(ref["path_cost"][qr]))
    assert np.array_equal(dev["paths"][q], ref["paths"][qr])


def test_64_queries_against_the_harness(big, harness):
    """1.  rtn, path_len, path_cost (as bits) and path_xyz identical for 64 queries; for 8 of them dist is exact wherever the true
    distance is <= the cost and >= the true distance elsewhere"""
    grid, starts, goals, gen = big
    dev = gen.grid_paths(starts, goals)
    print("device: %.3f ms, rounds %s, tile visits %s" % (gen.last_ms(), dev["stats"][:, 0].tolist(), dev["stats"][:, 1].tolist()))
    ref = gh.run(harness, grid, starts, goals, 4096, 0, sides=("early",), fields=False)["early"]
    for q in range(64):
        same_paths(dev, ref, q)
    assert (dev["rtn"] == cluster.GRID_PATH_OK).all() and dev["path_len"].min() > 60
    d8 = gen.grid_paths(starts[:8], goals[:8], want_dist=True)
    full = gh.run(harness, grid, starts[:8], goals[:8], 4096, 0, sides=("full",), fields=True)["full"]
    for q in range(8):
        same_paths(d8, full, q)
        same_paths(d8, dev, q)
        true, got, cost = full["dist"][q], d8["dist"][q], full["path_cost"][q]
        near = true <= cost
        print("query %d: cost %.3f, %d voxels within the cost, exact there: %s, never below elsewhere: %s"
              % (q, cost, near.sum(), np.array_equal(bits(got[near]), bits(true[near])), bool((got[~near] >= true[~near]).all())))
        assert np.array_equal(bits(got[near]), bits(true[near]))
        assert (got[~near] >= true[~near]).all()
        assert np.isposinf(got[grid.ravel() != 0]).all()


@pytest.mark.parametrize("case", gh.crafted_cases(), ids=lambda c: c["name"])
def test_crafted_cases(built, harness, case):
    """2.  every return code, partial tiles, a 2-D map, the maze, an occupied start, start == goal, a path_capacity that is too
    small; max_rounds = 1 ends a long query with ROUND_LIMIT while its neighbour in the batch is OK"""
    grid = case["grid"]
    gen = cluster.ClusterGenerator(grid.shape, max_batch=8, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
    dev = gen.grid_paths(case["starts"], case["goals"], path_capacity=case["cap"], max_rounds=case["max_rounds"], want_dist=True)
    gen.close()
    ref = gh.run(harness, grid, case["starts"], case["goals"], case["cap"], 0, sides=("full",), fields=True)["full"]
    if case["name"] == "tile_serpentine":
        # One tile, a path of more than 100 hops of which about 80 run along rows that one wave owns: a wave's lanes read before
        # any of them writes, so a sweep moves a value one hop there and the 64 sweeps of a visit cannot finish the tile.  It has
        # no neighbour: a second round can only come from the tile waking itself.
        print("one-tile serpentine: rounds %s, tile visits %s" % (dev["stats"][:, 0].tolist(), dev["stats"][:, 1].tolist()))
        assert (dev["stats"][:, 0] >= 2).all() and (dev["stats"][:, 1] == dev["stats"][:, 0]).all()
    for q in range(len(case["starts"])):
        want = case["rtn"][q] if case["rtn"] is not None else ref["rtn"][q]
        assert dev["rtn"][q] == want, (case["name"], q, dev["rtn"][q])
        if want == gh.ROUND_LIMIT:
            assert dev["path_len"][q] == 0 and np.isnan(dev["path_cost"][q]) and len(dev["paths"][q]) == 0
            continue
        same_paths(dev, ref, q)
        if want == gh.BAD_ENDPOINT:
            assert dev["path_len"][q] == 0 and np.isnan(dev["path_cost"][q])
            continue
        if want == gh.NO_PATH:
            assert dev["path_len"][q] == 0 and np.isposinf(dev["path_cost"][q])
            assert np.array_equal(bits(dev["dist"][q]), bits(ref["dist"][q]))  # the whole component of the start
        if want == gh.OVERFLOW:
            assert dev["path_len"][q] > case["cap"] and len(dev["paths"][q]) == case["cap"]
        if want in (gh.OK, gh.OVERFLOW):
            near = ref["dist"][q] <= ref["path_cost"][q]
            assert np.array_equal(bits(dev["dist"][q][near]), bits(ref["dist"][q][near]))
            assert (dev["dist"][q][~near] >= ref["dist"][q][~near]).all()


def test_launch_shape_independence(big):
    """3.  one call, two half calls and a permuted batch give identical bytes; so does a second call on the used workspace"""
    grid, starts, goals, gen = big

    def pack(r, order=None):
        n = len(r["paths"])
        order = range(n) if order is None else order
        xyz = np.zeros((n, 4096, 3), np.int32)
        for i, q in enumerate(order):
            xyz[i, :len(r["paths"][q])] = r["paths"][q]
        o = list(order)
        return xyz.tobytes() + r["path_len"][o].tobytes() + r["path_cost"][o].tobytes() + r["rtn"][o].tobytes()

    one = gen.grid_paths(starts, goals)
    again = gen.grid_paths(starts, goals)
    assert pack(one) == pack(again)
    h0, h1 = gen.grid_paths(starts[:32], goals[:32]), gen.grid_paths(starts[32:], goals[32:])
    halves = dict(paths=h0["paths"] + h1["paths"], **{k: np.concatenate([h0[k], h1[k]]) for k in ("path_len", "path_cost", "rtn")})
    assert pack(one) == pack(halves)
    perm = np.random.default_rng(1).permutation(64)
    p = gen.grid_paths(starts[perm], goals[perm])
    assert pack(one, perm) == pack(p)
    # the field, where the contract calls it exact, for 8 queries in three shapes
    a = gen.grid_paths(starts[:8], goals[:8], want_dist=True)
    b0, b1 = gen.grid_paths(starts[:4], goals[:4], want_dist=True), gen.grid_paths(starts[4:8], goals[4:8], want_dist=True)
    c = gen.grid_paths(starts[:8][::-1], goals[:8][::-1], want_dist=True)
    for q in range(8):
        near = a["dist"][q] <= a["path_cost"][q]
        other = (b0["dist"][q] if q < 4 else b1["dist"][q - 4])
        assert np.array_equal(bits(a["dist"][q][near]), bits(other[near]))
        assert np.array_equal(bits(a["dist"][q][near]), bits(c["dist"][7 - q][near]))
        assert ((c["dist"][7 - q] <= a["path_cost"][q]) == near).all()  # nothing else reaches below the cost


def test_device_memory_outputs(big):
    """4.  outputs in device memory equal outputs in host memory"""
    import torch
    grid, starts, goals, gen = big
    B, cap, G = 8, 300, grid.size
    s, g = np.ascontiguousarray(starts[:B]), np.ascontiguousarray(goals[:B])
    host = gen.grid_paths(s, g, path_capacity=cap, want_dist=True)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")
    xyz, n, cost = z((B, cap, 3), torch.int32), z(B, torch.int32), z(B, torch.float64)
    dist, stats, rtn = z((B, G), torch.float64), z((B, 2), torch.int32), z(B, torch.int32)
    torch.cuda.synchronize()
    st = cluster._lib().direct_cluster_grid_path_batch(gen.h, B, s.ctypes.data, g.ctypes.data, cap, 0, abi.MEM_DEVICE, xyz.data_ptr(),
                                                       n.data_ptr(), cost.data_ptr(), dist.data_ptr(), stats.data_ptr(), rtn.data_ptr())
    assert st == abi.DIRECT_OK
    n, xyz = n.cpu().numpy(), xyz.cpu().numpy()
    assert np.array_equal(n, host["path_len"]) and np.array_equal(rtn.cpu().numpy(), host["rtn"])
    assert np.array_equal(bits(cost.cpu().numpy()), bits(host["path_cost"]))
    for q in range(B):
        assert np.array_equal(xyz[q, :min(n[q], cap)], host["paths"][q])
        near = host["dist"][q] <= host["path_cost"][q]
        assert np.array_equal(bits(dist[q].cpu().numpy()[near]), bits(host["dist"][q][near]))
    # NULL outputs are left alone: only the codes
    only = np.full(B, -1, np.int32)
    st = cluster._lib().direct_cluster_grid_path_batch(gen.h, B, s.ctypes.data, g.ctypes.data, cap, 0, abi.MEM_HOST, None, None, None, None,
                                                       None, only.ctypes.data)
    assert st == abi.DIRECT_OK and np.array_equal(only, host["rtn"])


def test_resident_clusters_survive(built):
    """5.  polygon_generation_batch -> grid_path_batch -> hull_planes_batch(cluster_xyz = NULL): the planes are those of the same
    sequence without the path call"""
    RES, LOWER = 0.2, np.array([-12.0, -12.0, 0.0])
    grid, seeds = problems.make_voxel_map()
    seeds = seeds[:16]
    gen = cluster.ClusterGenerator(grid.shape, max_batch=16, cluster_capacity=50000, candidate_capacity=10000)
    gen.set_map(grid)
    free = np.argwhere(grid == 0)
    rng = np.random.default_rng(2)
    starts, goals = free[rng.integers(len(free), size=16)], free[rng.integers(len(free), size=16)]
    gen.polygon_generation(seeds, fetch_clusters=False)
    want = gen.hull_planes(RES, LOWER, batch=len(seeds))
    gen.polygon_generation(seeds, fetch_clusters=False)
    paths = gen.grid_paths(starts, goals, want_dist=True)
    got = gen.hull_planes(RES, LOWER, batch=len(seeds))
    gen.close()
    assert (paths["rtn"] == cluster.GRID_PATH_OK).sum() >= 8
    assert (want["rtn"] == cluster.HULL_OK).all()
    for k in ("rtn", "n_planes", "n_vertices", "degenerate", "center"):
        assert np.array_equal(want[k], got[k]), k
    for b in range(len(seeds)):
        for k in ("planes", "plane_int", "vertices"):
            assert np.array_equal(want[k][b], got[k][b]), (k, b)


def test_chain_into_the_corridor_generator(big, tmp_path):
    """6.  the device's paths, as voxel centres, through tests/cpp/test_corridor_gen.cpp (unchanged; the input format
    tests/real_corridor_lib.py writes): every walk succeeds, the start centre lies in the first polytope and the goal centre in
    the last (isOutsidePolytope's margin 0.01)"""
    from tests.real_corridor_lib import LOWER, RES
    grid, starts, goals, gen = big
    dev = gen.grid_paths(starts, goals)
    assert (dev["rtn"] == cluster.GRID_PATH_OK).all()
    paths = [p.astype(np.float64) * RES + 0.5 * RES + LOWER for p in dev["paths"]]
    fin, fout, exe = str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "gen")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3id3di", *grid.shape, RES, *LOWER, len(paths)))
        for p in paths:
            f.write(struct.pack("<i", len(p)))
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
        f.write(np.ascontiguousarray(grid, np.uint8).tobytes())
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests/cpp/test_corridor_gen.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "direct_amd/lib"), "-ldirect_ddp",
                           "-Wl,-rpath," + os.path.join(ROOT, "direct_amd/lib") + ":/opt/rocm/lib"])
    out = subprocess.run([exe, fin, fout, "64"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    raw, off = open(fout, "rb").read(), 0

    def take(fmt):
        nonlocal off
        v = struct.unpack_from(fmt, raw, off)
        off += struct.calcsize(fmt)
        return v

    inside = lambda c, planes: bool((planes[:, :3] @ c + planes[:, 3] <= 0.01).all())
    for mode in range(4):
        for p in range(len(paths)):
            ok, n = take("<2i")
            polys = []
            for _ in range(n):
                (k,) = take("<i")
                polys.append(np.array(take("<%dd" % (4 * k))).reshape(k, 4))
                take("<6d")
            assert ok == 1 and n >= 1, (mode, p)
            assert inside(paths[p][0], polys[0]), (mode, p)
            assert inside(paths[p][-1], polys[-1]), (mode, p)
    assert off == len(raw)
