"""Scenes that drive the corridor-cluster kernels into the code paths they pick by candidate count and cluster size -- TEST
INFRASTRUCTURE shared by tests/test_cluster_shell_scenes.py (CPU), tests/test_gpu_cluster.py and
tests/golden/make_cluster_golden.py.

A box of a x b x c free voxels whose six faces are each stopped by ONE obstacle voxel gives a first clustering round with
(a + 2)(b + 2)(c + 2) - a b c candidates (the free shell around the inflated cube) minus one per obstacle in that shell: the
candidate count is set by the box, and tuned to the voxel by the number of obstacles.  direct_cluster.hip switches code at
4096, 8192 and 16384 candidates per round (row words per lane of k_resolve_fast; k_resolve_pipe and the un-queued rows of
k_convex above 16384) and at 256 chunks of 256 cluster voxels.

Geometry.  The seed is the box's LOW corner (x0, y0, z0); the stoppers of the three low faces touch it, those of the three
high faces sit in the same corner column of their slabs: (x1 + 1, y0, z0), (x0, y1 + 1, z0), (x0, y0, z1 + 1).  A face's slab
has, while the cube grows, the ranges the cube has at that moment, and the corner column is in them from the start: the box
may have three different edge lengths (with the seed in the centre a short axis' corner stopper would not be in range yet when
its face arrives).  A stopper in a corner hides little: with stoppers at the face centres almost no candidate sees the whole
cluster.  The remaining obstacles of the first shell lie on its twelve EDGE rows.  Such a voxel is in the bounding box of a ray
from candidate to cluster voxel only for candidates of the same edge row (they fail the cluster test), and in the box of a
candidate-candidate ray only between the two shell planes that meet in the row (those candidates see the cluster and are
rejected by the chain): a few of either kind per obstacle, thousands of accepted candidates left.  Candidates are discovered in
the x, y, z order of the cube's surface, so the candidate index grows with x: edge obstacles are spread over the x-parallel
rows, and over the rows of both x-end planes, for every index range to hold some.  `outer` blockers two layers out act on the
second round only."""
import ctypes as C
import hashlib

import numpy as np

from oracle import clusterapi as ca

MARGIN = 6                      # free voxels between the box and the map's border, per side
RANGES = ((0, 4096), (4096, 8192), (8192, 16384), (16384, 1 << 30))   # 1 / 2 / 4 row words per lane, general kernels
MIN_ACCEPTED, MIN_CHAIN_REJECTED, MIN_CLUSTER_FAILED = 100, 3, 3      # the conditions on the inputs, per range
TAIL = 512                      # a range with fewer candidates is a boundary probe (unmet_conditions)
REPORT_COLUMNS = ("round", "lo", "hi", "sees", "accepted", "chain_rejected", "cluster_failed", "own_range")
ROUNDS = 2                      # itr_cluster_max of every scene


def shell_count(cube):
    a, b, c = cube
    return (a + 2) * (b + 2) * (c + 2) - a * b * c


def _edge_rows(lo, hi):
    """The twelve edge rows of the first shell as (axis, fixed coordinates): x-parallel rows first."""
    rows = []
    for axis in range(3):
        o1, o2 = [q for q in range(3) if q != axis]
        for s1 in (0, 1):
            for s2 in (0, 1):
                fixed = {o1: hi[o1] + 1 if s1 else lo[o1] - 1, o2: hi[o2] + 1 if s2 else lo[o2] - 1}
                rows.append((axis, fixed))
    return rows


def edge_obstacles(cube, n, layer=1):
    """n distinct voxels on the edge rows of the shell `layer` voxels out, in an order whose every prefix is spread over the
    rows and along them (golden-ratio sequence), at least three voxels from a row's ends (the stoppers sit at the corners)."""
    lo = np.array([MARGIN] * 3)
    hi = lo + np.array(cube) - 1
    rows = _edge_rows(lo - (layer - 1), hi + (layer - 1))
    out, seen, k = [], set(), 0
    while len(out) < n:
        axis, fixed = rows[k % 12]
        t = ((k // 12 + 1) * 0.6180339887498949 + 0.25 * (k % 12)) % 1.0
        if all(val > hi[q] for q, val in fixed.items()):
            t *= 0.4    # the three rows that meet in the high corner: its candidate is the round's LAST and walks half of each
        p = [0, 0, 0]
        p[axis] = int(lo[axis] + 3 + t * (cube[axis] - 6))
        for q, val in fixed.items():
            p[q] = int(val)
        k += 1
        if tuple(p) not in seen:
            seen.add(tuple(p))
            out.append(p)
        assert k < 100 * (n + 12), "edge rows exhausted"
    return np.array(out, np.int32).reshape(-1, 3)


def make_scene(name, cube, n_shell, n_outer=8):
    """-> dict(name, cube, n_shell, n_outer, grid, seed, box (x0, x1, y0, y1, z0, z1), surface, expect_candidates)."""
    cube = tuple(int(q) for q in cube)
    dims = tuple(q + 2 * MARGIN for q in cube)
    grid = np.zeros(dims, np.uint8)
    x0 = y0 = z0 = MARGIN
    x1, y1, z1 = x0 + cube[0] - 1, y0 + cube[1] - 1, z0 + cube[2] - 1
    for p in ((x0 - 1, y0, z0), (x0, y0 - 1, z0), (x0, y0, z0 - 1), (x1 + 1, y0, z0), (x0, y1 + 1, z0), (x0, y0, z1 + 1)):
        grid[p] = 1
    for p in edge_obstacles(cube, n_shell):
        assert grid[tuple(p)] == 0
        grid[tuple(p)] = 1
    for p in edge_obstacles(cube, n_outer, layer=2):
        grid[tuple(p)] = 1
    a, b, c = cube
    return dict(name=name, cube=cube, n_shell=int(n_shell), n_outer=int(n_outer), grid=grid, seed=np.array([x0, y0, z0], np.int32),
                box=(x0, x1, y0, y1, z0, z1), surface=a * b * c - max(a - 2, 0) * max(b - 2, 0) * max(c - 2, 0),
                expect_candidates=shell_count(cube) - 6 - int(n_shell))


# name, box, obstacles on the first shell's edge rows.  Three different edge lengths everywhere (a stride mix-up cannot hide);
# the boundary scenes are the same boxes with the obstacle count that leaves exactly that many first-round candidates.
def _boundary(cube, target):
    return shell_count(cube) - 6 - target


# The boxes above 8192 candidates are LONG in x.  The x-high plane of the shell is discovered last, and an obstacle in or around
# it hides plane candidates from candidates of lower index only; with a compact box the highest index range lies wholly inside
# that plane and every chain rejection in it is decided by accepted candidates of the ranges below (measured: 0 of 92 in
# [16384, n) of a 62 x 54 x 46 box).  A long box has a small end plane, the highest range holds several of the rings around the
# box with their edge-row obstacles, and some of its rejections are decided by accepted candidates of the range itself - the
# ones that need the upper words of the accepted bitset.
CUBE_S, CUBE_M, CUBE_L = (36, 28, 22), (90, 24, 20), (185, 24, 20)
SCENES = (
    ("s28", CUBE_S, 24), ("s38", CUBE_M, 40), ("s54", CUBE_L, 80),
    ("n4095", (30, 25, 21), None), ("n4096", (30, 25, 21), None), ("n4097", (30, 25, 21), None),
    ("n8192", (67, 28, 21), None), ("n8193", (67, 28, 21), None),
    ("n16384", (166, 25, 19), None), ("n16385", (166, 25, 19), None),
)


def scene(name):
    for nm, cube, k in SCENES:
        if nm == name:
            return make_scene(nm, cube, _boundary(cube, int(nm[1:])) if k is None else k)
    raise KeyError(name)


def scene_names():
    return [s[0] for s in SCENES]


def first_round_state(sc):
    """(vertex_idx, surface cluster, inside flags, first-round candidates) from the restatement: what
    direct_cluster_convex_test needs to repeat the first round's convex tests."""
    v, surf, _, rc = ca.polygon_generation(sc["grid"], sc["seed"], itr_cluster_max=0)
    assert rc == 0
    use, inside = ca.cube_state(sc["grid"], v)
    cand = ca.candidates(sc["grid"], use, np.zeros(sc["grid"].shape, np.uint8), inside, surf)
    return v, surf, inside, cand


def run_scene(sc, rounds=ROUNDS, reference=False, plug=True):
    """The clustering loop of the oracle round by round (cl_cluster_round), with every candidate classified.  reference=True
    runs the loop and the classification through the reference's own serialConvexTest (oracle/_ref); plug=False: the caller
    has plugged it in (run_scenes: the switch is one global of the oracle library).
    -> dict(vertex_idx, iters, sizes [cluster size after the surface and after every round], n_cand [per round], cluster,
            report [one row per round and index range])"""
    grid = np.ascontiguousarray(sc["grid"], np.uint8)
    dims = grid.shape
    L = ca.lib()
    fn_lib, fn_name = (ca.ref_lib(), "ref_serial_convex_test") if reference else (L, "cl_serial_convex_test")
    v, surf, _, rc = ca.polygon_generation(grid, sc["seed"], itr_cluster_max=0)
    assert rc == 0
    x0, x1, y0, y1, z0, z1 = sc["box"]
    assert (v[7], v[1], v[15], v[9], v[23], v[17]) == (x0, x1, y0, y1, z0, z1), "the stoppers did not shape the intended box"
    use, inside = ca.cube_state(grid, v)
    invalid = np.zeros(dims, np.uint8)
    cap = len(surf) + 27 * sum(shell_count(tuple(q + 2 * r for q in sc["cube"])) for r in range(rounds))
    cluster, active = np.zeros((cap, 3), np.int32), np.zeros((cap, 3), np.int32)
    cluster[:len(surf)] = active[:len(surf)] = surf
    n_clu, n_act = C.c_int(len(surf)), C.c_int(len(surf))
    scratch = np.zeros((cap, 3), np.int32)
    sizes, n_cand, report, iters = [len(surf)], [], [], 0
    if plug:
        ca.use_reference_convex_test(reference)
    try:
        for r in range(rounds):
            cand = ca.candidates(grid, use.copy(), invalid, inside, active[:n_act.value])
            if len(cand) == 0:
                break
            assert 26 * n_act.value <= cap
            before = n_clu.value
            done = L.cl_cluster_round(grid.ctypes.data, use.ctypes.data, invalid.ctypes.data, inside.ctypes.data, dims[0], dims[1],
                                      dims[2], cluster.ctypes.data, C.addressof(n_clu), active.ctypes.data, C.addressof(n_act),
                                      scratch.ctypes.data)
            n_cand.append(len(cand))
            sizes.append(n_clu.value)
            lin = lambda a: (a[:, 0] * dims[1] + a[:, 1]) * dims[2] + a[:, 2]
            accepted = np.isin(lin(cand), lin(cluster[before:n_clu.value]))
            assert accepted.sum() == n_clu.value - before
            # an accepted candidate saw the old cluster (serialConvexTest is an AND over targets); the others are asked
            can_clu = accepted.astype(np.uint8)
            rej = np.flatnonzero(~accepted)
            can_clu[rej] = ca.serial_convex_test(fn_lib, fn_name, cand[rej], cluster[:before], inside, grid, dims)
            assert np.array_equal(cand[accepted], cluster[before:n_clu.value])      # joined in candidate order
            for lo, hi in RANGES:
                if lo >= len(cand):
                    break
                s = slice(lo, min(hi, len(cand)))
                # chain rejections that only accepted candidates of index >= lo decide: the candidate sees every accepted
                # candidate below lo (the row words of the slots / registers before this range hold no hit for it)
                chain = lo + np.flatnonzero((can_clu[s] == 1) & ~accepted[s])
                below = cand[:lo][accepted[:lo]]
                own = int(ca.serial_convex_test(fn_lib, fn_name, cand[chain], below, inside, grid, dims).sum()) if lo else len(chain)
                report.append(dict(round=r, lo=lo, hi=min(hi, len(cand)), sees=int(can_clu[s].sum()), accepted=int(accepted[s].sum()),
                                   chain_rejected=len(chain), cluster_failed=int((can_clu[s] == 0).sum()), own_range=own))
            if not done:
                break
            iters += 1
    finally:
        if plug:
            ca.use_reference_convex_test(False)
    return dict(vertex_idx=v, iters=iters, sizes=np.array(sizes, np.int32), n_cand=np.array(n_cand, np.int32),
                cluster=cluster[:n_clu.value].copy(), report=report)


def run_scenes(names, reference=False, workers=4):
    """run_scene for several scenes on a few threads (the oracle's calls release the interpreter lock; the large scenes take
    a minute each) -> {name: result}"""
    from concurrent.futures import ThreadPoolExecutor
    names = sorted(names, key=lambda n: -int(np.prod(scene(n)["cube"])))      # longest first
    ca.use_reference_convex_test(reference)
    try:
        with ThreadPoolExecutor(max_workers=workers) as ex:
            out = list(ex.map(lambda n: run_scene(scene(n), reference=reference, plug=False), names))
    finally:
        ca.use_reference_convex_test(False)
    return dict(zip(names, out))


def format_report(name, res):
    lines = ["%s: candidates per round %s, cluster sizes %s, iters %d" % (name, res["n_cand"].tolist(), res["sizes"].tolist(), res["iters"])]
    for q in res["report"]:
        lines.append("  round %d [%5d, %5d): sees %5d  accepted %5d  chain-rejected %3d (%3d by their own range alone)  cluster-failed %4d"
                     % (q["round"], q["lo"], q["hi"], q["sees"], q["accepted"], q["chain_rejected"], q["own_range"], q["cluster_failed"]))
    return "\n".join(lines)


def unmet_conditions(res):
    """The conditions on the inputs, per index range in the FIRST round that reaches it.  The boundary scenes put one candidate
    past a threshold (n4097, n8193, n16385) or reach the next range with a thin tail in their second round: a range that holds
    fewer than TAIL candidates cannot be asked for a hundred accepted ones; there at least one candidate must be accepted, so
    that the range's words of the bitset are written at all.  Every range of the three main scenes holds more than TAIL.
    own_range - chain rejections that only accepted candidates of the range itself decide, the ones that need the range's
    own words of the accepted bitset - is asked (3 at least) of the HIGHEST full range of the first round: that is where the shell's
    x-high end plane and the rings next to it lie, whose candidates hide each other.  In a range in the middle of a long box
    a rejected candidate is, as a rule, also hidden from some far accepted candidate of a lower range along the same edge row
    (measured: 0 of 332 in [8192, 16384) of the 185-long box), and a second round's thin tail past a threshold lies wholly
    inside the end plane of the second shell (0 of 104 in [16384, 16970) of n16384), so each range gets its deciding scene: [4096, 8192) from s28,
    [8192, 16384) from s38 and n16384, [16384, n) from s54 (tests/test_cluster_shell_scenes.py asserts it)."""
    bad, seen = [], set()
    for q in res["report"]:
        if q["lo"] in seen:
            continue
        seen.add(q["lo"])
        if q["hi"] - q["lo"] < TAIL:
            if q["accepted"] < 1:
                bad.append(("tail range without an accepted candidate", q))
            continue
        top = q["round"] == 0 and q is [p for p in res["report"] if p["round"] == 0 and p["hi"] - p["lo"] >= TAIL][-1]
        if (q["accepted"] < MIN_ACCEPTED or q["chain_rejected"] < MIN_CHAIN_REJECTED or q["cluster_failed"] < MIN_CLUSTER_FAILED
                or (top and q["own_range"] < MIN_CHAIN_REJECTED)):
            bad.append(("conditions not met", q))
    return bad


def cluster_digest(cluster):
    return hashlib.sha256(np.ascontiguousarray(cluster, np.int32).tobytes()).hexdigest()


def with_side_rooms(sc):
    """The scene's map with two closed rooms in opposite corners of its margin, for batches that mix rows: a ONE-VOXEL pocket at
    the high corner (its three inner neighbours are obstacles) and a 3 x 3 x 3 room at the low corner behind walls at coordinate
    3; of its x wall only the stopper (3, 0, 0) stands, so its seed has eight candidates and some of them join.  Every added
    obstacle lies at a coordinate <= 3 or >= size - 2, outside the box [4, size - 5] of the scene's second shell: no ray of the
    scene's two rounds (a ray stays in the box of its two ends) meets one, and its result is the fixture's.
    -> (grid, pocket seed, room seed)"""
    grid = sc["grid"].copy()
    X, Y, Z = grid.shape
    for p in ((X - 2, Y - 1, Z - 1), (X - 1, Y - 2, Z - 1), (X - 1, Y - 1, Z - 2)):
        grid[p] = 1
    grid[:4, 3, :4] = 1
    grid[:4, :4, 3] = 1
    grid[3, 0, 0] = 1
    return grid, np.array([X - 1, Y - 1, Z - 1], np.int32), np.array([1, 1, 1], np.int32)


def explain(name, gold, got_cluster):
    """Where a device cluster leaves the fixture's: the first differing position, its round, and the scene's per-range report."""
    exp, sizes = gold[name + "_cluster"], gold[name + "_sizes"]
    n = min(len(exp), len(got_cluster))
    d = np.flatnonzero((exp[:n] != np.asarray(got_cluster)[:n]).any(1))
    first = int(d[0]) if len(d) else n
    rnd = int(np.searchsorted(sizes, first, "right")) - 1
    lines = ["%s: %d voxels against the fixture's %d; first difference at position %d = accepted candidate %d of round %d"
             % (name, len(got_cluster), len(exp), first, first - int(sizes[max(rnd, 0)]), rnd),
             "candidates per round %s, cluster sizes %s" % (gold[name + "_n_cand"].tolist(), sizes.tolist())]
    for q in gold[name + "_report"]:
        lines.append("  round %d [%5d, %5d): sees %5d  accepted %5d  chain-rejected %3d  cluster-failed %4d  own-range %3d" % tuple(int(v) for v in q))
    return "\n".join(lines)


def chunk_scene():
    """More than 256 chunks of 256 cluster voxels for direct_cluster_convex_test: a 48 x 44 x 36 map, the cluster = its first
    68000 free voxels in storage order (x up to 42; index 65536, where chunk 256 begins, is at x = 41), three dozen obstacles
    in the slabs behind the cluster and four on the low region's border edges (an obstacle in the middle of a cluster that fills
    the map hides something from every candidate).  Ten GATE obstacles at (41, 43, z) on the map's y border hide the cluster
    voxel (42, 43, z) behind them - one of the chunks from the 256th on - from the candidates put at (40, 43, z) and
    (39, 43, z) and from hardly anyone else (seen from a lower y the gate's shadow leaves the map): candidates that chunks
    256 .. 265 ALONE decide.  64 candidates, the others spread over the map; inside_data = a small box.
    -> dict(grid, inside, cand, cluster)"""
    rng = np.random.default_rng(17)
    dims = (48, 44, 36)
    grid = np.zeros(dims, np.uint8)
    obs = np.stack([rng.integers(43, 48, 36), rng.integers(0, 44, 36), rng.integers(0, 36, 36)], 1)
    grid[obs[:, 0], obs[:, 1], obs[:, 2]] = 1
    low = np.stack([rng.integers(0, 43, 4), rng.choice([0, 43], 4), rng.choice([0, 35], 4)], 1)
    grid[low[:, 0], low[:, 1], low[:, 2]] = 1
    gate = np.stack([np.full(10, 41), np.full(10, 43), 3 * np.arange(10) + 4], 1)
    grid[gate[:, 0], gate[:, 1], gate[:, 2]] = 1
    inside = np.zeros(dims, np.uint8)
    inside[20:26, 18:25, 15:20] = 1
    free = np.argwhere(grid == 0).astype(np.int32)           # storage (x, y, z) order
    cluster = free[:68000]
    cand = np.stack([rng.integers(0, d, 64) for d in dims], 1).astype(np.int32)
    cand[:10] = gate - [1, 0, 0]
    cand[10:14] = gate[:4] - [2, 0, 0]
    return dict(grid=grid, inside=inside, cand=cand, cluster=cluster)
