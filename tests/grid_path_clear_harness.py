"""The clear mode of the one program of tests/grid_path_harness.py (direct_amd/csrc/grid_path_clear_math.h compiled by g++) - TEST
INFRASTRUCTURE of tests/test_grid_path_clear_restatement.py, tests/test_gpu_grid_path_clear.py and tools/grid_path_clear_bench.py.
The C++ lives there; this module is build / run wrappers that send D2, the floor and the penalty table with the map.  Two sides
per query:
  full   that program's independent heap Dijkstra with the DEFINED cost written out - two rounded additions per move,
         (d(u) + w) + pen(v), the floor on D2, and the predecessor rule with the same two additions - none of it through the
         header's clearance functions;
  emu    its shared visit and walk with clear == true: "open" and the penalty fetched once per visit and voxel, the header's
         clear_candidate / accept / wake functions, and the header's clear_is_predecessor for the read-back.
A third side, early, is the Dijkstra of full left when the goal is popped: the sequential search the stage replaces, for the
benchmark's 64 queries on the large map (its field is exact wherever the true distance is <= the path's cost).
All report the contract's return codes, path_d2 and path_min_d2.  Also here: a brute-force NumPy distance field and the maps
the CPU and the GPU tests share."""
import numpy as np

from tests import grid_path_harness as gh

ROOT = gh.ROOT
OK, NO_PATH, BAD_ENDPOINT, OVERFLOW, ROUND_LIMIT = gh.OK, gh.NO_PATH, gh.BAD_ENDPOINT, gh.OVERFLOW, gh.ROUND_LIMIT
DIST_NONE = 0x7fffffff
SIDES = ("full", "emu", "early")


def build(workdir, local_iters=None):
    """local_iters: a build with fewer sweeps per tile visit than the library's (DIRECT_GRIDPATH_LOCAL_ITERS), so that small maps
    reach the branch in which a tile runs out of sweeps and wakes itself"""
    return gh.build_program(workdir, local_iters)


def run(harness, grid, d2, starts, goals, min_d2=0, penalty=None, path_capacity=4096, max_rounds=0, sides=("full", "emu"), fields=True):
    """-> {side: dict(rtn, path_len, path_cost, stats, path_min_d2, paths: list of [n][3], path_d2: list of [n], dist [nq][G] or None)}"""
    return gh.run_pairs(harness, ("rtn", "path_len", "path_cost", "stats", "path_min_d2", "paths", "path_d2", "dist"),
                        [s for s in SIDES if s in sides], grid, starts, goals, path_capacity, max_rounds, fields,
                        clear=True, d2=d2, min_d2=min_d2, penalty=penalty)


def brute_distance_field(grid, cap_vox=0):
    """min(D2, cap2) by brute force: for every voxel the smallest squared distance to a voxel with byte 1 (int32, DIST_NONE on a
    map without one; cap2 = cap_vox^2, or none for cap_vox == 0) - the definition of direct_cluster_distance_field"""
    grid = np.asarray(grid)
    occ = np.argwhere(grid == 1).astype(np.int64)
    out = np.full(grid.size, DIST_NONE, np.int64)
    if len(occ):
        vox = np.stack(np.unravel_index(np.arange(grid.size), grid.shape), axis=1).astype(np.int64)
        for a in range(0, len(vox), 512):
            diff = vox[a:a + 512, None, :] - occ[None, :, :]
            out[a:a + 512] = (diff * diff).sum(axis=2).min(axis=1)
    if cap_vox > 0:
        out = np.minimum(out, cap_vox * cap_vox)
    return out.reshape(grid.shape).astype(np.int32)


# ---- the maps the CPU and the GPU tests share: 40 x 24 x 12, five tiles along x, partial tiles along z -----------------------

def walls_map():
    """walls across x, full height, seven voxels apart, each with a gap 7 voxels wide along y (its middle column has D2 = 16) and
    the first four with a second, narrower gap of width 1, 2, 3 and 5 (middle D2 = 1, 1, 4, 9) elsewhere: a floor on D2 closes the
    narrow gaps one after the other and the paths move to the wide ones"""
    g = np.zeros((40, 24, 12), np.uint8)
    for x, wide, narrow in ((6, 15, (3, 1)), (13, 1, (18, 2)), (20, 14, (4, 3)), (27, 2, (17, 5)), (34, 10, None)):
        g[x, :, :] = 1
        g[x, wide:wide + 7, :] = 0
        if narrow:
            g[x, narrow[0]:narrow[0] + narrow[1], :] = 0
    g[0:3, 0, 0] = 1   # a clutter row next to the corner: voxels below a floor that are not walls
    return g


def gap_map():
    """one thick wall across x with a direct gap one voxel wide (y = 12, full height) and a wide opening far off (y = 0 .. 4):
    the unpenalised optimum squeezes through the gap, a proximity penalty pays for the detour through open space"""
    g = np.zeros((40, 24, 12), np.uint8)
    g[18:22, :, :] = 1
    g[18:22, 12, :] = 0
    g[18:22, 0:5, :] = 0
    g[8, 8:16, 3:9] = 1    # two plates the paths skirt on either side of the wall
    g[31, 9:17, 2:8] = 1
    return g


def queries(grid, d2, n, seed, floor=0):
    """n (start, goal) pairs of free voxels with D2 >= floor on opposite sides of the map along x"""
    rng = np.random.default_rng(seed)
    ok = (grid == 0) & (d2 >= floor)
    left, right = np.argwhere(ok[:5]), np.argwhere(ok[35:]) + [35, 0, 0]
    s, g = left[rng.integers(len(left), size=n)], right[rng.integers(len(right), size=n)]
    swap = rng.random(n) < 0.5
    s[swap], g[swap] = g[swap].copy(), s[swap].copy()
    return s.astype(np.int32), g.astype(np.int32)


def soft_table(weight=0.3, radius=4.0):
    """the table of the penalty cases: weight * (1 - sqrt(d2) / radius)^2 below radius^2, non-representable doubles"""
    d2 = np.arange(int(np.ceil(radius * radius)), dtype=np.float64)
    return weight * (1.0 - np.sqrt(d2) / radius) ** 2
