"""direct_cluster_hull_planes_batch (include/direct_cluster.h; poly_utils.cpp:127-206, 282-389) on the device against the
oracle (oracle/hull_ref.c, pinned against the reference's quickhull by tests/test_hull.py): planes, lattice planes,
corners and centre bit for bit; committed quickhull golden vectors; device-resident chaining seeds -> clusters ->
planes -> DDP; the shapes of tests/hull_shape_lib.py (large extents, shells, flat discs, capacities, reuse, optional outputs)
against the oracle results committed in tests/golden/hull_shapes.npz."""
import os

import numpy as np
import pytest

from direct_amd import abi, cluster, problems, solver
from oracle import clusterapi, hullapi
from tests import hull_shape_lib as shapes

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RES, LOWER = 0.2, np.array([-12.0, -12.0, 0.0])


def same(dev, b, ref):
    assert dev["rtn"][b] == ref["rc"] and dev["degenerate"][b] == ref["degenerate"]
    assert dev["n_planes"][b] == ref["n_planes"] and dev["n_vertices"][b] == ref["n_vertices"]
    assert np.array_equal(dev["plane_int"][b], ref["plane_int"])
    assert np.array_equal(dev["planes"][b], ref["planes"])          # doubles, bit for bit (same IEEE operations)
    assert np.array_equal(dev["vertices"][b], ref["vertices"])
    assert np.array_equal(dev["center"][b], ref["center"])


def test_hull_planes_match_the_oracle_and_the_quickhull_golden(built):
    g = np.load(os.path.join(GOLD, "hull_quickhull_16.npz"))
    clusters = [g["cluster_%d" % i] for i in range(int(g["n"]))]
    gen = cluster.ClusterGenerator((64, 64, 32), max_batch=len(clusters), cluster_capacity=8192, candidate_capacity=64)
    dev = gen.hull_planes(RES, LOWER, clusters=clusters)
    for b, cl in enumerate(clusters):
        ref = hullapi.hull_planes(cl, RES, LOWER)
        same(dev, b, ref)
        vq = np.rint((dev["vertices"][b] - LOWER) / (RES / 2)).astype(np.int64)
        hullapi.check_mesh(g["qh_vertices_%d" % b], g["qh_triangles_%d" % b], dev["plane_int"][b], vq)
    gen.close()


def test_hull_of_device_resident_clusters_and_edge_cases(built):
    grid, seeds = problems.make_voxel_map()
    seeds = seeds[:24]
    gen = cluster.ClusterGenerator(grid.shape, max_batch=32, cluster_capacity=50000, candidate_capacity=10000)
    gen.set_map(grid)
    r = gen.polygon_generation(seeds)
    dev = gen.hull_planes(RES, LOWER, batch=len(seeds))                 # no voxel leaves or enters the device
    for b in range(len(seeds)):
        same(dev, b, hullapi.hull_planes(r["clusters"][b], RES, LOWER))
    assert (dev["n_planes"] >= 6).all() and dev["n_planes"].max() > 12
    # caller-provided clusters: empty, one voxel, a flat slab, a diagonal sheet (not full-dimensional), capacity overflow
    cases = [np.zeros((0, 3), np.int32), np.array([[4, 4, 5]]), np.array([[x, y, 5] for x in range(3, 9) for y in range(4, 7)]),
             np.array([[x, x, z] for x in range(5) for z in range(4)]), r["clusters"][0]]
    dev = gen.hull_planes(RES, LOWER, clusters=cases, plane_capacity=8)
    assert list(dev["rtn"][:4]) == [cluster.HULL_FLAT, cluster.HULL_OK, cluster.HULL_OK, cluster.HULL_FLAT]
    for b in (1, 2):
        same(dev, b, hullapi.hull_planes(cases[b], RES, LOWER, plane_cap=8))
    full = hullapi.hull_planes(cases[4], RES, LOWER)
    assert dev["rtn"][4] == cluster.HULL_OVERFLOW and dev["n_planes"][4] == full["n_planes"]
    assert np.array_equal(dev["plane_int"][4], full["plane_int"][:8])
    gen.close()


def grid_path(grid, start, goal):
    """a 4-connected shortest voxel path at the height of `start` (breadth first), as voxel-centre coordinates"""
    from collections import deque
    z = start[2]
    free = grid[:, :, z] == 0
    prev = -np.ones(free.shape + (2,), np.int32)
    seen = np.zeros(free.shape, bool)
    dq = deque([(int(start[0]), int(start[1]))])
    seen[start[0], start[1]] = True
    while dq:
        x, y = dq.popleft()
        if (x, y) == (int(goal[0]), int(goal[1])):
            break
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            u, v = x + dx, y + dy
            if 0 <= u < free.shape[0] and 0 <= v < free.shape[1] and free[u, v] and not seen[u, v]:
                seen[u, v] = True
                prev[u, v] = (x, y)
                dq.append((u, v))
    assert seen[goal[0], goal[1]]
    path, cur = [], (int(goal[0]), int(goal[1]))
    while cur != (int(start[0]), int(start[1])):
        path.append(cur)
        cur = tuple(int(c) for c in prev[cur])
    path.append(cur)
    return np.array([[x, y, z] for x, y in path[::-1]], np.float64) * RES + 0.5 * RES + LOWER


def test_corridor_generation_walk_and_ddp(built, tmp_path):
    """corridorGeneration (poly_utils.cpp:508-557) and corridorInsertGeneration (:391-449, the live caller's walk,
    teach_repeat_planner.cpp:172 / 228) through the C++ host class (direct_amd/host/poly_utils.hpp): grid
    paths -> corridors, path by path and all paths in lock step, against the walk restated over the CPU checkers
    (planes bit for bit); then the corridor is what the DDP path consumes: the replay batch of one of them is solved."""
    import struct
    import subprocess
    from direct_amd import corridor_io
    from oracle import corridor_walk
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    grid, _ = problems.make_voxel_map()
    free = np.argwhere(grid[:, :, 8] == 0)
    rng = np.random.default_rng(4)
    paths = []
    while len(paths) < 5:
        a, b = free[rng.integers(len(free))], free[rng.integers(len(free))]
        if np.abs(a - b).sum() > 60:
            try:
                paths.append(grid_path(grid, [a[0], a[1], 8], [b[0], b[1], 8]))
            except AssertionError:
                pass
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3id3di", *grid.shape, RES, *LOWER, len(paths)))
        for p in paths:
            f.write(struct.pack("<i", len(p)))
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
        f.write(np.ascontiguousarray(grid, np.uint8).tobytes())
    exe = str(tmp_path / "test_corridor_gen")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(root, "tests/cpp/test_corridor_gen.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "direct_amd/lib"), "-ldirect_ddp",
                           "-Wl,-rpath," + os.path.join(root, "direct_amd/lib") + ":/opt/rocm/lib"])
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert out.returncode == 0 and "PASS" in out.stdout, out.stdout + out.stderr
    raw = open(fout, "rb").read()
    off = 0

    def take(fmt):
        nonlocal off
        v = struct.unpack_from(fmt, raw, off)
        off += struct.calcsize(fmt)
        return v
    cache, modes = {}, []
    want = [corridor_walk.corridor_generation(grid, RES, LOWER, p, cache=cache) for p in paths]
    want_ins = []  # corridorInsertGeneration (poly_utils.cpp:391-449): first half into an empty corridor, second half into that
    for p in paths:
        c1, r1 = corridor_walk.corridor_insert_generation(grid, RES, LOWER, p[:len(p) // 2], [], cache=cache)
        c2, r2 = corridor_walk.corridor_insert_generation(grid, RES, LOWER, p[len(p) // 2:], c1, cache=cache)
        want_ins.append((c2, r1 == 1 and r2 == 1))
    for mode in range(4):
        got = []
        for p in range(len(paths)):
            ok, n = take("<2i")
            cor = []
            for _ in range(n):
                (k,) = take("<i")
                pl = np.array(take("<%dd" % (4 * k))).reshape(k, 4)
                cor.append(dict(planes=pl, center=np.array(take("<3d")), seed_coord=np.array(take("<3d"))))
            got.append((cor, bool(ok)))
        modes.append(got)
    assert off == len(raw)
    n_poly = 0
    # the insert walk never pops: on these paths it keeps polytopes the plain walk drops again
    assert sum(len(c) for c, _ in want_ins) >= sum(len(c) for c, _ in want)
    for mi, got in enumerate(modes):
        for (gc, gok), (wc, wok) in zip(got, want if mi < 2 else want_ins):
            assert gok == wok and len(gc) == len(wc) and len(gc) >= 2
            for a, b in zip(gc, wc):
                assert np.array_equal(a["planes"], b["planes"]) and np.array_equal(a["center"], b["center"])
                assert np.array_equal(a["seed_coord"], b["seed_coord"])
            n_poly += len(gc)
    # the corridor feeds the DDP path: wire format -> replay batch (first n polytopes, n = 2 ..) -> two-phase plan
    cor = max((c for c, _ in modes[1] if max(len(q["planes"]) for q in c) <= abi.P_LIMIT), key=len)   # P_LIMIT 54: all of them
    assert len(cor) >= 3
    pm = max(len(q["planes"]) for q in cor)
    planes = np.zeros((len(cor), pm, 4))
    for i, q in enumerate(cor):
        planes[i, :len(q["planes"])] = q["planes"]
    c = corridor_io.Corridor(7, [len(q["planes"]) for q in cor], planes, [q["seed_coord"] for q in cor], [q["center"] for q in cor])
    c2, _ = corridor_io.unpack(corridor_io.pack(c), 64, pm)
    assert np.array_equal(c2.planes, c.planes)
    batch = corridor_io.replay_batch(c2, n_first=2)
    s = solver.DdpSolver(batch.batch, int(batch.n_seg.max()), pm, np.float64)
    g0, g1 = s.plan(abi.phase0_params(), abi.phase1_params(), batch)
    d = s.sample(batch.n_seg, g1.bez, g1.T, 0.05, 4096, derivs=0, n_planes=batch.n_planes, planes=batch.planes)
    s.close()
    assert (g1.rtn >= 0).any()
    assert (d["cmax"][g1.rtn >= 0] < 1e-6).all()       # solved trajectories stay inside their polytopes


def test_hull_input_guards(built):
    """(a) a caller-provided voxel outside the map disqualifies ITS cluster (DIRECT_HULL_BAD_VOXEL) instead of
    addressing lattice lines outside the per-cluster arrays, the other clusters of the call are unaffected; (b) the
    resident-cluster form needs a generation of at least `batch` seeds, and caller-provided voxels - which are packed
    into the handle's cluster storage - retire the resident clusters; (c) a generation that overflowed the cluster
    capacity in a clustering round keeps the valid PREFIX of the cluster (every returned voxel is a map voxel of the
    oracle's cluster, in its order) and its hull is refused (DIRECT_HULL_OVERFLOW) rather than computed on slots that
    were never written."""
    from direct_amd.solver import DirectError
    grid, seeds = problems.make_voxel_map()
    gen = cluster.ClusterGenerator(grid.shape, max_batch=8, cluster_capacity=20000, candidate_capacity=4000)
    gen.set_map(grid)
    r = gen.polygon_generation(seeds[:3])
    assert (r["rtn"] == cluster.CLUSTER_OK).all()
    good = gen.hull_planes(RES, LOWER, batch=3)
    assert (good["rtn"] == cluster.HULL_OK).all()
    # (b) more clusters than the last generation produced
    with pytest.raises(DirectError) as e:
        gen.hull_planes(RES, LOWER, batch=4)
    assert e.value.status == abi.DIRECT_ERR_INVALID
    # (a) one voxel of cluster 1 outside the map, in every direction the packing could alias
    for badv in ([-1, 3, 3], [grid.shape[0], 2, 2], [3, 3, 1024 + 5], [2, grid.shape[1] + 7, 1]):
        cl = [c.copy() for c in r["clusters"]]
        cl[1][len(cl[1]) // 2] = badv
        h = gen.hull_planes(RES, LOWER, clusters=cl)
        assert h["rtn"][1] == cluster.HULL_BAD_VOXEL and h["n_planes"][1] == 0
        for b in (0, 2):
            assert h["rtn"][b] == cluster.HULL_OK and np.array_equal(h["planes"][b], good["planes"][b])
    # (b) the caller's voxels replaced the resident clusters: a resident call needs a new generation
    with pytest.raises(DirectError):
        gen.hull_planes(RES, LOWER, batch=3)
    gen.close()
    # (c) overflow in a clustering round: capacity just above the inflated cube's surface
    _, cl_full, _, _ = clusterapi.polygon_generation(grid, tuple(int(v) for v in seeds[0]))
    gen = cluster.ClusterGenerator(grid.shape, max_batch=2, cluster_capacity=len(cl_full) - 5, candidate_capacity=4000)
    gen.set_map(grid)
    ro = gen.polygon_generation(seeds[:1])
    assert ro["rtn"][0] == cluster.CLUSTER_OVERFLOW
    n = int(ro["cluster_num"][0])
    assert 0 < n <= len(cl_full) - 5
    assert np.array_equal(ro["clusters"][0], cl_full[:n])          # a valid prefix, never stale storage
    ho = gen.hull_planes(RES, LOWER, batch=1)
    assert ho["rtn"][0] == cluster.HULL_OVERFLOW and ho["n_planes"][0] == 0
    gen.close()


# ---- shapes beyond grown blobs (tests/hull_shape_lib.py; oracle results committed in tests/golden/hull_shapes.npz) ----
CCAP = 20480          # holds the R = 30.5 shell (20024 voxels); box_cap fills it exactly
SMALL = [n for n, s in shapes.SHAPES.items() if s[1] == shapes.SMALL_MAP]
CAPS = dict(plane_capacity=shapes.PLANE_CAP, vertex_capacity=shapes.VERT_CAP)


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLD, "hull_shapes.npz"))


def small_gen(max_batch):
    return cluster.ClusterGenerator(shapes.SMALL_MAP, max_batch=max_batch, cluster_capacity=CCAP, candidate_capacity=64)


def rows_equal(a, i, b, j):
    """row i of call a and row j of call b are the same answer (only what the call defines: n_planes planes, n_vertices corners)"""
    for k in ("rtn", "degenerate", "n_planes", "n_vertices"):
        assert a[k][i] == b[k][j], k
    for k in ("plane_int", "planes", "vertices"):
        assert np.array_equal(a[k][i], b[k][j]), k
    if a["rtn"][i] == cluster.HULL_OK:
        assert np.array_equal(a["center"][i], b["center"][j])


def test_shapes_match_the_committed_oracle_bitwise(built, fix):
    """Voxel shells (hundreds of candidates and planes), flat discs in z, x and y above the 256-point chunk of k_hull_cand
    and of the corner compaction, a disc one voxel away from flat, the diagonal sheet, a cluster that fills the capacity, and
    the shell with more line-extreme points than hull::kCandCap in the middle of them: one call, every row bit for bit."""
    names = SMALL[:9] + [shapes.OVERFLOW_SHAPE] + SMALL[9:]
    gen = small_gen(len(names))
    dev = gen.hull_planes(RES, LOWER, clusters=[shapes.build(n) for n in names], **CAPS)
    gen.close()
    for b, n in enumerate(names):
        shapes.assert_same(shapes.device_row(dev, b), shapes.fixture_row(fix, n), n)
    b = names.index(shapes.OVERFLOW_SHAPE)
    assert dev["rtn"][b] == cluster.HULL_OVERFLOW and dev["n_planes"][b] == 0 and dev["n_vertices"][b] == 0


def test_one_call_with_every_return_code_equals_the_rows_alone(built, fix):
    ball, shell = shapes.build("ball_6.5"), shapes.build(shapes.OVERFLOW_SHAPE)
    bad = ball.copy()
    bad[len(bad) // 3] = [shapes.SMALL_MAP[0], 2, 2]
    cases = [ball, shapes.build("disc_25.5_z"), shapes.sheet(), bad, shell, np.zeros((0, 3), np.int32), ball, shapes.box_cap()]
    num = [len(c) for c in cases]
    num[6], num[7] = -3, CCAP + 7                    # below zero: an empty row; above the capacity: clamped to it
    assert len(cases[7]) == CCAP
    gen = small_gen(len(cases))
    dev = gen.hull_planes(RES, LOWER, clusters=cases, num=num, **CAPS)
    gen.close()
    assert list(dev["rtn"]) == [cluster.HULL_OK, cluster.HULL_OK, cluster.HULL_FLAT, cluster.HULL_BAD_VOXEL, cluster.HULL_OVERFLOW,
                                cluster.HULL_FLAT, cluster.HULL_FLAT, cluster.HULL_OK]
    for b, n in ((0, "ball_6.5"), (1, "disc_25.5_z"), (2, "sheet"), (4, shapes.OVERFLOW_SHAPE), (7, "box_cap")):
        shapes.assert_same(shapes.device_row(dev, b), shapes.fixture_row(fix, n), n)
    for b in (3, 5, 6):
        assert dev["n_planes"][b] == 0 and dev["n_vertices"][b] == 0
    one = small_gen(1)
    for b in range(len(cases)):
        rows_equal(dev, b, one.hull_planes(RES, LOWER, clusters=[cases[b]], num=[num[b]], **CAPS), 0)
    one.close()


def test_a_reused_handle_answers_like_a_fresh_one(built, fix):
    """Slot 0 holds the R = 10.5 shell (344 candidates, 192 corners), then a 3 x 3 x 3 box (8 candidates), then a flat disc
    (56 candidates of which 32 are corners): lattice lines, first partners and corner flags of the earlier call must be gone."""
    box = np.array([[x, y, z] for x in range(4, 7) for y in range(5, 8) for z in range(2, 5)])
    seq = [(shapes.build("ball_10.5"), shapes.fixture_row(fix, "ball_10.5")), (box, hullapi.hull_planes(box, RES, LOWER)),
           (shapes.build("disc_10.5_z"), shapes.fixture_row(fix, "disc_10.5_z"))]
    gen = small_gen(2)
    for cl, ref in seq:
        dev = gen.hull_planes(RES, LOWER, clusters=[cl], **CAPS)
        shapes.assert_same(shapes.device_row(dev, 0), ref)
        fresh = small_gen(2)
        rows_equal(dev, 0, fresh.hull_planes(RES, LOWER, clusters=[cl], **CAPS), 0)
        fresh.close()
    gen.close()


def test_capacities_count_only_for_outputs_that_were_asked_for(built, fix):
    cl, ref = shapes.build("ball_10.5"), shapes.fixture_row(fix, "ball_10.5")
    assert ref["n_vertices"] == 192 and ref["n_planes"] == 122
    gen = small_gen(1)
    # vertex capacity below the corner count: reported, the count exact, the corners that fit and all planes delivered
    d = gen.hull_planes(RES, LOWER, clusters=[cl], plane_capacity=shapes.PLANE_CAP, vertex_capacity=100)
    assert d["rtn"][0] == cluster.HULL_OVERFLOW and d["n_vertices"][0] == 192 and d["n_planes"][0] == 122
    assert np.array_equal(d["vertices"][0], ref["vertices"][:100])
    assert np.array_equal(d["plane_int"][0], ref["plane_int"]) and np.array_equal(d["planes"][0], ref["planes"])
    assert np.array_equal(d["center"][0], ref["center"])
    # the same without the vertices: their capacity does not count
    d = gen.hull_planes(RES, LOWER, clusters=[cl], plane_capacity=shapes.PLANE_CAP, vertex_capacity=100,
                        want=("planes", "plane_int", "center"))
    assert d["rtn"][0] == cluster.HULL_OK and d["n_vertices"][0] == 192 and d["vertices"] is None
    assert np.array_equal(d["plane_int"][0], ref["plane_int"]) and np.array_equal(d["planes"][0], ref["planes"])
    assert np.array_equal(d["center"][0], ref["center"])
    # neither planes nor plane_int: the plane capacity does not count, the plane count stays exact
    d = gen.hull_planes(RES, LOWER, clusters=[cl], plane_capacity=8, vertex_capacity=shapes.VERT_CAP, want=("vertices", "center"))
    assert d["rtn"][0] == cluster.HULL_OK and d["n_planes"][0] == 122 and d["n_vertices"][0] == 192
    assert np.array_equal(d["vertices"][0], ref["vertices"]) and np.array_equal(d["center"][0], ref["center"])
    # plane_int alone still makes the capacity count
    d = gen.hull_planes(RES, LOWER, clusters=[cl], plane_capacity=8, vertex_capacity=shapes.VERT_CAP, want=("plane_int",))
    assert d["rtn"][0] == cluster.HULL_OVERFLOW and d["n_planes"][0] == 122
    assert np.array_equal(d["plane_int"][0], ref["plane_int"][:8])
    gen.close()


def test_clusters_as_wide_as_the_largest_map_match_the_oracle(built, fix):
    """Extents of 255 .. 1022 voxels on a 1023 x 1023 x 64 map, with the pair on either side of the extent at which
    hull::edge_test's tie-break product left 64 bits (hull_shape_lib).  The handle: 0.27 GB summed-area table, 67 MB map and
    scratch copy, and per batch row 67 MB of flags, 268 MB of keys and 38 MB of lattice lines: 1.2 GB at max_batch 2, allocated
    and never touched apart from the lines (two fills of 75 MB per call)."""
    gen = cluster.ClusterGenerator(shapes.BIG_MAP, max_batch=2, cluster_capacity=16, candidate_capacity=64)
    for i in range(0, len(shapes.EXTENT), 2):
        names = shapes.EXTENT[i:i + 2]
        dev = gen.hull_planes(RES, LOWER, clusters=[shapes.build(n) for n in names], **CAPS)
        for b, n in enumerate(names):
            ref = shapes.fixture_row(fix, n)
            assert ref["rc"] == 0 and ref["n_planes"] == 6 and ref["n_vertices"] == 8
            shapes.assert_same(shapes.device_row(dev, b), ref, n)
    gen.close()
