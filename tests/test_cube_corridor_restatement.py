"""direct_amd/csrc/cube_corridor_math.h (the arithmetic of direct_cluster_cube_corridor_batch), built by g++
(tests/cube_corridor_harness.py), against three witnesses that share no code with it:
  cube    a NumPy transcription of cubeInflation_cpu's literal loop nest, which reads the map bytes slab by slab and tests > 0
          (polyhedron_generator/src/cluster_server_cpu.cpp:126-293), where the header asks the summed-area table;
  planes  the host build of the hull phases (tests/emu/, as tests/test_hull.py drives it), fed the cube's surface voxels in
          k_inflate's order: planes and centre bit for bit;
  walk    a Python port of polyhedronGenerator::walk (direct_amd/host/poly_utils.hpp) run on those cubes and planes.
Then the named cases: each asserts that what its name says really happens on the shared map."""
import numpy as np
import pytest

from tests import cube_corridor_harness as ch
from tests.emu import hullemu

RES, LOWER = ch.RES, ch.LOWER


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("cube_corridor"))


# ---- witness 1: the loop nest on the map bytes ---------------------------------------------------------------------------
def loop_nest_cube(grid, seed, itr_inflate_max):
    X, Y, Z = grid.shape
    x0 = x1 = int(seed[0]); y0 = y1 = int(seed[1]); z0 = z1 = int(seed[2])
    for _ in range(itr_inflate_max):
        last = (x0, x1, y0, y1, z0, z1)
        if y0 != 0 and not (grid[x0:x1 + 1, y0 - 1, z0:z1 + 1] > 0).any():
            y0 -= 1
        if y1 != Y - 1 and not (grid[x0:x1 + 1, y1 + 1, z0:z1 + 1] > 0).any():
            y1 += 1
        if x0 != 0 and not (grid[x0 - 1, y0:y1 + 1, z0:z1 + 1] > 0).any():
            x0 -= 1
        if x1 != X - 1 and not (grid[x1 + 1, y0:y1 + 1, z0:z1 + 1] > 0).any():
            x1 += 1
        if z0 != 0 and not (grid[x0:x1 + 1, y0:y1 + 1, z0 - 1] > 0).any():
            z0 -= 1
        if z1 != Z - 1 and not (grid[x0:x1 + 1, y0:y1 + 1, z1 + 1] > 0).any():
            z1 += 1
        if last == (x0, x1, y0, y1, z0, z1):
            break
    return [x0, y0, z0, x1, y1, z1]


def axis_by_axis_cube(grid, seed):
    """NOT the definition: every direction grown as far as it goes before the next one is looked at"""
    X, Y, Z = grid.shape
    lo, hi = [int(v) for v in seed], [int(v) for v in seed]
    dims = (X, Y, Z)

    def slab(a, at):
        sl = [slice(lo[k], hi[k] + 1) for k in range(3)]
        sl[a] = at
        return grid[tuple(sl)]

    moved = True
    while moved:
        moved = False
        for a in (1, 0, 2):
            while lo[a] > 0 and not slab(a, lo[a] - 1).any():
                lo[a] -= 1
                moved = True
            while hi[a] < dims[a] - 1 and not slab(a, hi[a] + 1).any():
                hi[a] += 1
                moved = True
    return lo + hi


@pytest.mark.parametrize("density", [0.02, 0.08, 0.3])
def test_cube_of_every_seed_against_the_loop_nest(harness, density):
    grid = ch.random_map(int(density * 1000), density)
    seeds = np.argwhere(np.ones(ch.DIMS, bool)).astype(np.int32)
    for itr in (1, 2, 1000):
        got, queries = ch.cubes(harness, grid, seeds, itr)
        want = np.array([loop_nest_cube(grid, s, itr) for s in seeds], np.int32)
        assert np.array_equal(got, want), (density, itr, np.argwhere((got != want).any(axis=1))[:4])
        rounds = sum(ch.DIMS)  # every round that goes on moves a face
        assert queries.max() <= 6 * (min(itr, rounds) + 1) and queries.min() >= 0
    assert grid.any() and (grid[tuple(seeds.T)] == 1).any()  # occupied seeds are among them: their byte is not looked at


def test_cube_is_defined_on_the_table_bytes_equal_to_one(harness):
    """set_map does not validate: a byte of 2 is an obstacle to the reference's `> 0` and none to the table's `== 1`.  The header
    follows the table; on maps of 0 and 1 the two agree (the test above)."""
    grid = np.zeros(ch.DIMS, np.uint8)
    grid[10, 10, 5] = 2
    got, _ = ch.cubes(harness, grid, [[4, 10, 5]])
    assert got[0].tolist() == [0, 0, 0, 23, 19, 11]
    assert loop_nest_cube(grid, [4, 10, 5], 1000) != got[0].tolist()


# ---- witness 2: the hull checker on the cube's surface voxels -----------------------------------------------------------------
def surface_cluster(c):
    """the cluster k_inflate leaves for a cube: its surface voxels in x, y, z order (the one voxel of a one-voxel cube)"""
    x0, y0, z0, x1, y1, z1 = [int(v) for v in c]
    return np.array([[x, y, z] for x in range(x0, x1 + 1) for y in range(y0, y1 + 1) for z in range(z0, z1 + 1)
                     if x in (x0, x1) or y in (y0, y1) or z in (z0, z1)], np.int32)


def shape_cubes():
    cubes = [[5, 6, 7, 5, 6, 7]]                                                            # the single voxel
    cubes += [[2, 3, 4, 9, 3, 4], [2, 3, 4, 2, 8, 4], [2, 3, 4, 2, 3, 9]]                     # lines along x, y, z
    cubes += [[1, 2, 3, 1, 7, 9], [1, 2, 3, 6, 2, 9], [1, 2, 3, 6, 7, 3]]                     # flat along x, y, z
    cubes += [[0, 0, 0, 1, 1, 1], [0, 0, 0, 23, 19, 11], [3, 1, 2, 4, 9, 5], [7, 7, 7, 20, 8, 8]]  # solid
    return cubes


def test_planes_and_centre_against_the_hull_checker(harness):
    cubes = shape_cubes()
    for density in (0.02, 0.3):
        grid = ch.random_map(int(density * 1000), density)
        seeds = np.argwhere(np.ones(ch.DIMS, bool)).astype(np.int32)[:: 97]
        cubes += np.unique(ch.cubes(harness, grid, seeds)[0], axis=0).tolist()
    for res, lower in ((RES, LOWER), (0.01, np.array([0.3, -0.7, 1.1]))):
        planes, center, deg = ch.polytopes(harness, cubes, res, lower)
        for i, c in enumerate(cubes):
            r = hullemu.hull_planes(surface_cluster(c), res, lower)
            assert r["rc"] == 0 and r["n_planes"] == 6 and r["n_vertices"] == 8, c
            assert r["degenerate"] == deg[i] == int(c[0] == c[3] or c[1] == c[4] or c[2] == c[5]), c
            assert np.array_equal(bits(r["planes"]), bits(planes[i])), c
            assert np.array_equal(bits(r["center"]), bits(center[i])), c
    assert sum(d == 1 for d in deg) >= 7 and sum(d == 0 for d in deg) >= 10


# ---- witness 3: the host walk -----------------------------------------------------------------------------------------------
def host_walk(path, planes_of, res, lower, pop_back):
    """polyhedronGenerator::walk for one path from an empty corridor -> the path indices of the corridor's polytopes"""
    def outside(cur, pl):
        return any(cur[0] * p[0] + cur[1] * p[1] + cur[2] * p[2] + p[3] > 0.01 for p in pl)

    cor, lst = [], None
    for i, idx in enumerate(path):
        cur = [int(idx[a]) * res + 0.5 * res + float(lower[a]) for a in range(3)]
        if cur == lst:
            continue
        if pop_back and len(cor) > 1 and not outside(cur, planes_of(cor[-2])):
            cor.pop()
        if not cor or outside(cur, planes_of(cor[-1])):
            cor.append(i)
        lst = cur
    return cor


def check_against_host_walk(harness, grid, paths, res, pop_back, seg_capacity=40):
    xyz, n = ch.pack_paths(paths)
    got = ch.corridors(harness, grid, xyz, n, res=res, pop_back=pop_back, seg_capacity=seg_capacity)
    for b, p in enumerate(paths):
        p = np.asarray(p, np.int32)
        cube, _ = ch.cubes(harness, grid, p)
        planes, center, _ = ch.polytopes(harness, cube, res, LOWER)
        cor = host_walk(p, lambda i: planes[i].tolist(), res, LOWER, pop_back)
        assert got["rtn"][b] == ch.OK and got["n_seg"][b] == len(cor), (b, cor)
        k = len(cor)
        assert np.array_equal(got["cube_idx"][b, :k], cube[cor])
        assert np.array_equal(bits(got["planes"][b, :k]), bits(planes[cor]))
        assert np.array_equal(bits(got["centers"][b, :k]), bits(center[cor]))
        seeds = np.array([[int(p[i][a]) * res + 0.5 * res + float(LOWER[a]) for a in range(3)] for i in cor]).reshape(-1, 3)
        assert np.array_equal(bits(got["seeds"][b, :k]), bits(seeds))
        assert (got["n_planes"][b, :k] == 6).all()
        for key in ("n_planes", "planes", "seeds", "centers", "cube_idx"):
            assert not got[key][b, k:].any(), key
    return got


@pytest.mark.parametrize("pop_back", [True, False])
def test_walk_against_the_host_walk(harness, pop_back):
    popped = 0
    for density, res in ((0.02, RES), (0.08, RES), (0.3, RES), (0.08, 0.01)):
        grid = ch.random_map(int(density * 1000), density)
        paths = ch.random_paths(grid, 24, seed=int(density * 100) + pop_back)
        got = check_against_host_walk(harness, grid, paths, res, pop_back)
        other = ch.corridors(harness, grid, *ch.pack_paths(paths), res=res, pop_back=not pop_back, seg_capacity=40)
        popped += int((got["n_seg"] != other["n_seg"]).sum())
    assert popped > 0  # the two variants differ somewhere on these paths


# ---- the named cases ----------------------------------------------------------------------------------------------------------
CASES = {c["name"]: c for c in ch.named_cases()}


def run_case(harness, name, **kw):
    c = CASES[name]
    grid = ch.crafted_map()
    xyz, n = ch.pack_paths(c["paths"])
    args = dict(res=c["res"], pop_back=c["pop_back"], seg_capacity=c["seg_capacity"])
    args.update(kw)
    return grid, c, ch.corridors(harness, grid, xyz, n, **args)


def stopped_by(grid, cube):
    """per side (lo x, lo y, lo z, hi x, hi y, hi z): 'border', 'obstacle', or None (a cube that is not a fixpoint)"""
    lo, hi, out = list(cube[:3]), list(cube[3:]), []
    for side in range(6):
        a, up = side % 3, side >= 3
        at = hi[a] + 1 if up else lo[a] - 1
        if at < 0 or at >= grid.shape[a]:
            out.append("border")
            continue
        sl = [slice(lo[k], hi[k] + 1) for k in range(3)]
        sl[a] = at
        out.append("obstacle" if grid[tuple(sl)].any() else None)
    return out


def test_named_faces_stopped_by_obstacles_and_by_the_border(harness):
    for name, what in (("obstacle_faces", "obstacle"), ("border_faces", "border")):
        grid, c, got = run_case(harness, name)
        check_against_host_walk(harness, grid, c["paths"], c["res"], c["pop_back"])
        seen = set()
        for b in range(len(c["paths"])):
            for k in range(got["n_seg"][b]):
                s = stopped_by(grid, got["cube_idx"][b, k])
                assert None not in s
                seen |= {i for i in range(6) if s[i] == what}
        assert seen == set(range(6)), (name, seen)


def test_named_round_order_enclosed_thin_and_occupied(harness):
    grid, c, got = run_case(harness, "round_order")
    seed = c["paths"][0][0]
    assert got["cube_idx"][0, 0].tolist() == loop_nest_cube(grid, seed, 1000) != axis_by_axis_cube(grid, seed)
    grid, c, got = run_case(harness, "enclosed_seed")
    assert got["n_seg"][0] == 1 and got["cube_idx"][0, 0].tolist() == [13, 4, 4, 13, 4, 4]
    grid, c, got = run_case(harness, "thin_corridor")
    cube = got["cube_idx"][0, 0]
    assert cube[1] == cube[4] == 12 and cube[2] == cube[5] == 5 and cube[3] - cube[0] >= 9  # one voxel thick along y and z
    check_against_host_walk(harness, grid, c["paths"], c["res"], c["pop_back"])
    grid, c, got = run_case(harness, "occupied_seed")
    cube = got["cube_idx"][0, 0]
    assert grid[17, 17, 9] == 1 and (cube[:3] <= [17, 17, 9]).all() and (cube[3:] >= [17, 17, 9]).all() and cube[3] > cube[0]
    check_against_host_walk(harness, grid, c["paths"], c["res"], c["pop_back"])


def test_named_repeated_points_and_single_voxel(harness):
    grid, c, got = run_case(harness, "repeated_points")
    p = np.array(c["paths"][0])
    keep = [0] + [i for i in range(1, len(p)) if (p[i] != p[i - 1]).any()]
    assert len(keep) < len(p)
    once = ch.corridors(harness, grid, *ch.pack_paths([p[keep]]), res=c["res"], pop_back=True, seg_capacity=32)
    for key in ("n_seg", "planes", "seeds", "centers", "cube_idx", "rtn"):
        assert np.array_equal(got[key], once[key]), key
    check_against_host_walk(harness, grid, c["paths"], c["res"], True)
    grid, c, got = run_case(harness, "single_voxel_path")
    assert got["n_seg"][0] == 1 and got["rtn"][0] == ch.OK
    assert got["cube_idx"][0, 0].tolist() == loop_nest_cube(grid, c["paths"][0][0], 1000)


def test_named_u_turn_with_and_without_pop_back(harness):
    grid, c, pop = run_case(harness, "u_turn")
    _, _, keep = run_case(harness, "u_turn_no_pop")
    check_against_host_walk(harness, grid, c["paths"], c["res"], True)
    check_against_host_walk(harness, grid, c["paths"], c["res"], False)
    assert pop["n_seg"][0] < keep["n_seg"][0]           # the way back removes polytopes instead of adding them
    n = pop["n_seg"][0]
    assert np.array_equal(pop["cube_idx"][0, :n], keep["cube_idx"][0, :n])


def test_named_resolution_where_the_threshold_decides(harness):
    """at resolution 0.01 a centre one voxel outside the cube is 0.005 beyond its plane, inside the 0.01 margin: the walk goes on where
    the same path at resolution 0.2 starts a polytope"""
    grid, c, fine = run_case(harness, "resolution_0.01")
    _, _, coarse = run_case(harness, "resolution_0.01", res=RES)
    check_against_host_walk(harness, grid, c["paths"], 0.01, True)
    voxel = lambda r, res: np.rint((r["seeds"][0, 1] - LOWER) / res - 0.5).astype(int).tolist()
    # the room's cube ends at x = 7: the coarse walk starts its second polytope at the door (8, 5, 5), one voxel outside; the fine
    # walk passes over the door and starts it at (9, 5, 5)
    assert coarse["cube_idx"][0, 0].tolist() == fine["cube_idx"][0, 0].tolist() == [3, 3, 3, 7, 7, 7]
    assert voxel(coarse, RES) == [8, 5, 5] and voxel(fine, 0.01) == [9, 5, 5]
    assert not np.array_equal(coarse["cube_idx"][0, 1], fine["cube_idx"][0, 1])


def test_named_capacity_and_outside_voxel(harness):
    grid, c, _ = run_case(harness, "seg_capacity_short", seg_capacity=32)
    full = ch.corridors(harness, grid, *ch.pack_paths(c["paths"]), res=c["res"], pop_back=c["pop_back"], seg_capacity=32)
    need = int(full["n_seg"].max())
    assert (full["rtn"] == ch.OK).all() and need >= 3 and full["n_seg"][1] < need
    cut = ch.corridors(harness, grid, *ch.pack_paths(c["paths"]), res=c["res"], pop_back=c["pop_back"], seg_capacity=need - 1)
    assert cut["rtn"].tolist() == c["rtn"] and np.array_equal(cut["n_seg"], full["n_seg"])
    for key in ("n_planes", "planes", "seeds", "centers", "cube_idx"):
        assert np.array_equal(cut[key], full[key][:, :need - 1]), key
    grid, c, got = run_case(harness, "outside_voxel")
    assert got["rtn"].tolist() == c["rtn"]
    bad = got["rtn"] == ch.BAD_PATH
    assert not got["n_seg"][bad].any() and not got["planes"][bad].any() and not got["n_planes"][bad].any()
    alone = ch.corridors(harness, grid, *ch.pack_paths([c["paths"][1]]), res=c["res"], pop_back=True, seg_capacity=32)
    assert np.array_equal(alone["planes"][0], got["planes"][1]) and alone["n_seg"][0] == got["n_seg"][1] > 0
