"""Time of direct_cluster_free_components and direct_cluster_reachable_batch, in one process, timed by direct_cluster_last_ms (HIP
events), median of 20 calls after 3 warm-up calls each, on three maps: the 200 x 200 x 40 map of tools/grid_path_bench.py, the launch
file's 333 x 333 x 33 map (a dense cloud, margin 0.25 m) and the plan check's 1024 x 1024 x 16 map:
  (a) the build at min_d2 0, and at a floor of 9 on the resident distance field;
  (b) direct_amd/csrc/free_comp_math.h on one host thread (g++ -O2, tests/free_comp_harness.py) on the same maps: its labels, sizes
      and stats must equal the device's byte for byte;
and on the 200 x 200 x 40 map, where the path benches have their queries, with ONE sealed pocket added to it (a closed shell of
occupied voxels around one free voxel):
  (c) direct_cluster_grid_path_batch with the bench's 64 queries;
  (d) a fan call of 4096 goals from one source, one of them the voxel in the pocket: enterable, unreachable;
  (e) the same fan call with the goals reachable() does not foretell OK removed, and the time of that reachable call;
  (d near), (e near) the same two calls with the 4095 other goals drawn within 24 voxels of the source: the case in which the
      fan's pruning bound has something to prune, and the pocket goal switches it off.
The aims, both against figures of this run: (a) below (c), and (a) + reachable + (e) below (d).  Every step that uses the device
runs under a time limit of its own (SIGALRM with the default action: the process ends there and starts nothing more).
usage: free_comp_bench.py [out.json] [builds]   (default profiles/free_comp_bench.json; "builds": (a) and (b) only, nothing is
       written - the run to repeat under a kernel trace for the per-kernel times)"""
import contextlib
import json
import os
import signal
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402,F401  (before the library is loaded)
from direct_amd import cluster, problems  # noqa: E402
from tests import free_comp_harness as fh  # noqa: E402
from tests import grid_path_harness as gh  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "free_comp_bench.json")
CALLS, WARM, NQ, NG, CAP, FLOOR = 20, 3, 64, 4096, 1024, 9


@contextlib.contextmanager
def limit(seconds):
    signal.alarm(seconds)
    yield
    signal.alarm(0)


def timed(gen, call):
    ms = []
    for _ in range(WARM + CALLS):
        r = call()
        ms.append(gen.last_ms())
    ms = ms[WARM:]
    return r, dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4), ms_max=round(float(max(ms)), 4))


def launch_map():
    res, lower = 0.15, np.array([-25.0, -25.0, 0.0])
    dims = tuple(int(v * (1.0 / res)) for v in (50.0, 50.0, 5.0))
    gen = cluster.ClusterGenerator(dims, max_batch=1, cluster_capacity=64, candidate_capacity=64)
    gen.set_map_from_cloud(problems.make_point_cloud(dims, res, lower, seed=11, n_points=1000000), lower, res, 0.25)
    grid = gen.get_map()
    gen.close()
    return grid


def pocket_map():
    """the path bench's map with a sealed pocket: the first 3 x 3 x 3 block of free voxels away from the border becomes a shell"""
    grid = gh.big_map().copy()
    for x, y, z in np.argwhere(grid[101:-3, 1:-3, 1:-3] == 0) + np.array([101, 1, 1]):
        if not grid[x:x + 3, y:y + 3, z:z + 3].any():
            grid[x:x + 3, y:y + 3, z:z + 3] = 1
            grid[x + 1, y + 1, z + 1] = 0
            return grid, np.array([x + 1, y + 1, z + 1], np.int32)
    raise AssertionError("no room for a pocket")


exe = fh.build(tempfile.mkdtemp(prefix="free_comp_bench_"))
with limit(120):
    pocket, pocket_voxel = pocket_map()
    maps = (("path_bench_200x200x40_pocket", pocket), ("launch_file_333x333x33", launch_map()),
            ("plan_check_1024x1024x16", problems.make_voxel_map((1024, 1024, 16), seed=7, n_pillars=1000, n_boxes=400, n_rings=100)[0]))

builds = []
for name, grid in maps:
    grid = np.ascontiguousarray(grid, np.uint8)
    with limit(240):
        gen = cluster.ClusterGenerator(grid.shape, max_batch=1, cluster_capacity=64, candidate_capacity=64)
        gen.set_map(grid)
        gen.build_distance_field()
        d2 = gen.distance_field()
    for floor in (0, FLOOR):
        with limit(240):
            host = fh.run(exe, grid, d2, floor)
            stats, t = timed(gen, lambda: gen.build_free_components(floor))
            label, size = gen.free_components()
            fh.assert_same(dict(label=label, size=size, stats=np.array([stats[k] for k in ("enterable", "components", "largest", "largest_label")])),
                           host["label"], host["size"], host["stats"], (name, floor))
        row = dict(map=name, dims=list(grid.shape), min_d2=floor, device=t, host_one_thread_ms=round(float(host["host_ms"]), 3),
                   speedup=round(float(host["host_ms"]) / t["ms_median"], 1), cross_tile_unions=host["unions"], **stats)
        builds.append(row)
        print("(a, b) %-30s min_d2 %d: %9d enterable in %6d components (largest %9d); device %.3f ms (min %.3f, max %.3f); one host thread %.1f ms"
              % (name, floor, stats["enterable"], stats["components"], stats["largest"], t["ms_median"], t["ms_min"], t["ms_max"], host["host_ms"]),
              flush=True)
    gen.close()
if sys.argv[2:3] == ["builds"]:
    sys.exit(0)

# ---- the filter in front of the path calls, on the path bench's map with the pocket ---------------------------------------
grid = pocket
starts, goals64 = gh.big_queries(gh.big_map(), NQ)
ok = (grid[tuple(starts.T)] == 0) & (grid[tuple(goals64.T)] == 0)
assert ok.all(), "the pocket's shell took an endpoint of the bench's queries"
free = np.argwhere(grid == 0)
goals4k = free[np.random.default_rng(17).integers(len(free), size=NG)].astype(np.int32)
goals4k[NG // 2] = pocket_voxel
source = starts[:1].copy()
with limit(120):
    gen = cluster.ClusterGenerator(grid.shape, max_batch=NQ, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
with limit(300):
    _, row_a = timed(gen, lambda: gen.build_free_components())
    pair, row_c = timed(gen, lambda: gen.grid_paths(starts, goals64, path_capacity=CAP))
    assert (gen.reachable(starts, goals64)[0] == cluster.GRID_PATH_OK).all() and (pair["rtn"] != cluster.GRID_PATH_NO_PATH).all()
with limit(300):
    full, row_d = timed(gen, lambda: gen.grid_paths_fan(source, goals4k, path_capacity=CAP))
    reach, row_r = timed(gen, lambda: gen.reachable(np.repeat(source, NG, axis=0), goals4k))
    keep = reach[0] == cluster.GRID_PATH_OK
    assert np.array_equal(keep, np.isin(full["rtn"], (cluster.GRID_PATH_OK, cluster.GRID_PATH_OVERFLOW))) and not keep[NG // 2]
    assert reach[2][NG // 2] == 1 and full["rtn"][NG // 2] == cluster.GRID_PATH_NO_PATH
    part, row_e = timed(gen, lambda: gen.grid_paths_fan(source, goals4k[keep], path_capacity=CAP))
    kept = np.flatnonzero(keep)
    assert np.array_equal(part["rtn"], full["rtn"][kept]) and np.array_equal(part["path_cost"].view(np.int64), full["path_cost"][kept].view(np.int64))
    assert all(np.array_equal(part["paths"][i], full["paths"][j]) for i, j in enumerate(kept))
with limit(300):
    near_vox = free[np.abs(free - source[0]).max(axis=1) <= 24]
    near = near_vox[np.random.default_rng(18).integers(len(near_vox), size=NG)].astype(np.int32)
    near[NG // 2] = pocket_voxel
    full_n, row_dn = timed(gen, lambda: gen.grid_paths_fan(source, near, path_capacity=CAP))
    keep_n = gen.reachable(np.repeat(source, NG, axis=0), near)[0] == cluster.GRID_PATH_OK
    part_n, row_en = timed(gen, lambda: gen.grid_paths_fan(source, near[keep_n], path_capacity=CAP))
    assert keep_n.sum() == NG - 1 and np.array_equal(part_n["rtn"], full_n["rtn"][keep_n])
    assert np.array_equal(part_n["path_cost"].view(np.int64), full_n["path_cost"][keep_n].view(np.int64))
gen.close()
for tag, row, what in (("a", row_a, "build, min_d2 0"), ("c", row_c, "grid_paths, 64 queries"), ("d", row_d, "fan, 4096 goals, one in the pocket"),
                       ("r", row_r, "reachable, 4096 pairs"), ("e", row_e, "fan, %d goals left by reachable" % keep.sum()),
                       ("d near", row_dn, "fan, 4095 goals within 24 voxels + pocket"), ("e near", row_en, "fan, those 4095 goals alone")):
    print("(%s) %-40s %.3f ms (min %.3f, max %.3f)" % (tag, what, row["ms_median"], row["ms_min"], row["ms_max"]), flush=True)
filtered = round(row_a["ms_median"] + row_r["ms_median"] + row_e["ms_median"], 4)
filtered_n = round(row_a["ms_median"] + row_r["ms_median"] + row_en["ms_median"], 4)
aims = dict(build_below_pairwise=bool(row_a["ms_median"] < row_c["ms_median"]), filtered_fan_ms=filtered,
            filtered_fan_below_fan=bool(filtered < row_d["ms_median"]), near_filtered_fan_ms=filtered_n,
            near_filtered_fan_below_fan=bool(filtered_n < row_dn["ms_median"]))
print("aims: (a) %.3f < (c) %.3f: %s; (a) + reachable + (e) = %.3f < (d) %.3f: %s"
      % (row_a["ms_median"], row_c["ms_median"], aims["build_below_pairwise"], filtered, row_d["ms_median"], aims["filtered_fan_below_fan"]), flush=True)
print("near goals: (a) + reachable + (e near) = %.3f < (d near) %.3f: %s" % (filtered_n, row_dn["ms_median"], aims["near_filtered_fan_below_fan"]), flush=True)

res = dict(calls=CALLS, warmup=WARM, device=torch.cuda.get_device_name(0), floor=FLOOR, builds=builds,
           filter=dict(map=list(grid.shape), pocket_voxel=pocket_voxel.tolist(), source=source[0].tolist(), path_capacity=CAP, goals=NG,
                       goals_kept=int(keep.sum()), a_build=row_a, c_grid_paths_64=row_c, d_fan_with_pocket_goal=row_d, reachable=row_r,
                       e_fan_filtered=row_e, d_near_fan_with_pocket_goal=row_dn, e_near_fan_filtered=row_en, aims=aims))
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"free_comp_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"free_comp_bench": dict(builds={"%s/%d" % (r["map"], r["min_d2"]): r["device"]["ms_median"] for r in builds}, a=row_a["ms_median"],
                                          c=row_c["ms_median"], d=row_d["ms_median"], reachable=row_r["ms_median"], e=row_e["ms_median"], **aims)}))
