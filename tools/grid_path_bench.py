"""Time of direct_cluster_grid_path_batch for 64 queries on the 200 x 200 x 40 map of tests/real_corridor_lib.py, timed by
direct_cluster_last_ms (HIP events): median of 20 calls after warm-up, rounds and tile visits.  Two reference points measured
in the same run on the same machine:
  (a) the sequential search the stage replaces: a heap Dijkstra with the same weights that stops when the goal is popped
      (tests/grid_path_harness.py, g++ -O2), one host thread, per query;
  (b) the next stage of the chain: direct_cluster_last_ms of generating the polytopes of those same 64 corridors - the 64
      corridors are walked in lock step; a round generates the cluster of every unfinished path's current voxel
      (polygon_generation_batch) and its planes (hull_planes_batch on the resident clusters), and every path then moves on to
      its first voxel outside the new polytope (isOutsidePolytope's margin 0.01).  The times of all rounds are summed.
usage: grid_path_bench.py [out.json]   (default profiles/grid_path_bench.json)"""
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
from direct_amd import cluster  # noqa: E402
from tests import grid_path_harness as gh  # noqa: E402
from tests.real_corridor_lib import LOWER, RES  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "grid_path_bench.json")
CALLS, WARM, NQ = 20, 3, 64

grid = gh.big_map()
starts, goals = gh.big_queries(grid, NQ)
gen = cluster.ClusterGenerator(grid.shape, max_batch=NQ, cluster_capacity=50000, candidate_capacity=10000)
gen.set_map(grid)
ms = []
for _ in range(WARM + CALLS):
    r = gen.grid_paths(starts, goals)
    ms.append(gen.last_ms())
assert (r["rtn"] == cluster.GRID_PATH_OK).all()
ms = ms[WARM:]

# (a) the sequential search, and a check of the device's paths against it on the way
ref = gh.run(gh.build(tempfile.mkdtemp()), grid, starts, goals, 4096, 0, sides=("early",), fields=False)["early"]
assert all(np.array_equal(r["paths"][q], ref["paths"][q]) for q in range(NQ))
assert np.array_equal(r["path_cost"].view(np.int64), ref["path_cost"].view(np.int64))

# (b) the polytopes of the same corridors
centres = [p.astype(np.float64) * RES + 0.5 * RES + LOWER for p in r["paths"]]
pos = np.zeros(NQ, np.int64)
gen_ms = hull_ms = 0.0
rounds = polytopes = failed = excluded = 0
while True:
    live = [q for q in range(NQ) if pos[q] < len(centres[q])]
    if not live:
        break
    seeds = np.array([r["paths"][q][pos[q]] for q in live], np.int32)
    g = gen.polygon_generation(seeds, fetch_clusters=False)
    gen_ms += gen.last_ms()
    h = gen.hull_planes(RES, LOWER, batch=len(live))
    hull_ms += gen.last_ms()
    rounds += 1
    for i, q in enumerate(live):
        if g["rtn"][i] != cluster.CLUSTER_OK or h["rtn"][i] != cluster.HULL_OK:  # no polytope from this voxel: the next one
            failed += 1
            pos[q] += 1
            continue
        polytopes += 1
        pl = h["planes"][i]
        out = (centres[q][pos[q]:] @ pl[:, :3].T + pl[:, 3] > 0.01).any(axis=1)
        excluded += int(out[0])  # a polytope whose planes exclude its own seed centre: counted, the walk goes on
        pos[q] += max(1, int(np.argmax(out)) if out.any() else len(out))
gen.close()

res = dict(queries=NQ, map=list(grid.shape), calls=CALLS, ms_median=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4),
           ms_max=round(float(max(ms)), 4), rounds_max=int(r["stats"][:, 0].max()), rounds_mean=round(float(r["stats"][:, 0].mean()), 2),
           tile_visits_total=int(r["stats"][:, 1].sum()), tile_visits_max=int(r["stats"][:, 1].max()),
           path_voxels_mean=round(float(r["path_len"].mean()), 1), path_cost_mean=round(float(r["path_cost"].mean()), 3),
           host_dijkstra_goal_exit_ms_sum=round(float(ref["ms"].sum()), 2), host_dijkstra_goal_exit_ms_median_per_query=round(float(np.median(ref["ms"])), 3),
           next_stage_polytopes_ms=round(gen_ms + hull_ms, 3), next_stage_generation_ms=round(gen_ms, 3), next_stage_hull_ms=round(hull_ms, 3),
           next_stage_rounds=rounds, next_stage_polytopes=polytopes, next_stage_seeds_without_polytope=failed,
           next_stage_polytopes_excluding_their_seed=excluded)
res["under_next_stage"] = bool(res["ms_median"] < res["next_stage_polytopes_ms"])
print("grid paths, %d queries: %.3f ms (min %.3f, max %.3f), up to %d rounds, %d tile visits; host Dijkstra with goal exit: %.1f ms for all "
      "(median %.2f per query); polytopes of the same corridors: %.2f ms in %d rounds (%d polytopes)"
      % (NQ, res["ms_median"], res["ms_min"], res["ms_max"], res["rounds_max"], res["tile_visits_total"], res["host_dijkstra_goal_exit_ms_sum"],
         res["host_dijkstra_goal_exit_ms_median_per_query"], res["next_stage_polytopes_ms"], rounds, polytopes), flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"grid_path_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"grid_path_bench": res}))
