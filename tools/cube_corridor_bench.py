"""Time of direct_cluster_cube_corridor_batch for the 64 queries of tools/grid_path_bench.py on the 200 x 200 x 40 map, in one
process, timed by direct_cluster_last_ms (HIP events), median of 20 calls after 3 warm-up calls each:
  (a) the grid path call (device outputs);
  (b) the way to the same corridors that exists beside the new call: polyhedronGenerator::walk in lock step with
      (itr_inflate_max, itr_cluster_max) = (1000, 0) - every round one polygon_generation_batch for the seeds that are due and one
      hull_planes_batch on the resident clusters; a call's time is the sum over its rounds (host time between them not counted);
  (c) the new call on the device-resident paths of (a).
(b) and (c) must agree bit for bit on every row (b) completes; (c) must equal the g++ build of its arithmetic
(tests/cube_corridor_harness.py), which also counts the table queries per cube.
usage: cube_corridor_bench.py [out.json]   (default profiles/cube_corridor_bench.json)"""
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402,F401  (before the library is loaded)
from direct_amd import abi, cluster  # noqa: E402
from tests import cube_corridor_harness as ch  # noqa: E402
from tests import grid_path_harness as gh  # noqa: E402
from tests.real_corridor_lib import LOWER, RES  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "cube_corridor_bench.json")
CALLS, WARM, NQ, CAP, SEG = 20, 3, 64, 4096, 64

grid = gh.big_map()
starts, goals = gh.big_queries(grid, NQ)
gen = cluster.ClusterGenerator(grid.shape, max_batch=NQ, cluster_capacity=50000, candidate_capacity=10000)
gen.set_map(grid)

# (a)
ms_a = []
for _ in range(WARM + CALLS):
    dev = gen.grid_paths(starts, goals, path_capacity=CAP, mem="device")
    ms_a.append(gen.last_ms())
assert (dev["rtn"].cpu().numpy() == cluster.GRID_PATH_OK).all()
path_len = dev["path_len"].cpu().numpy()
paths = [dev["path_xyz"][q, :path_len[q]].cpu().numpy() for q in range(NQ)]

# (c)
ms_c = []
for _ in range(WARM + CALLS):
    cor = gen.cube_corridors(dev["path_xyz"], dev["path_len"], LOWER, RES, pop_back=True, seg_capacity=SEG)
    ms_c.append(gen.last_ms())
cor = {k: v.cpu().numpy() for k, v in cor.items()}
assert (cor["rtn"] == cluster.CUBE_CORRIDOR_OK).all()
want = ch.corridors(ch.build(tempfile.mkdtemp()), grid, dev["path_xyz"].cpu().numpy(), path_len, res=RES, lower=LOWER, seg_capacity=SEG)
for k in abi.CUBE_CORRIDOR_OUTPUTS:
    assert cor[k].tobytes() == want[k].tobytes(), k
queries = np.concatenate([want["queries"][q, :path_len[q]] for q in range(NQ)])


# (b)
def lock_step():
    def outside(cur, pl):
        return bool((pl[:, 0] * cur[0] + pl[:, 1] * cur[1] + pl[:, 2] * cur[2] + pl[:, 3] > 0.01).any())

    centres = [p.astype(np.float64) * RES + 0.5 * RES + LOWER for p in paths]
    walks = [[] for _ in range(NQ)]
    nxt, failed, ms, rounds, made = [0] * NQ, [False] * NQ, 0.0, 0, 0
    while True:
        due = []
        for q in range(NQ):
            while not failed[q] and nxt[q] < len(paths[q]):   # (consecutive voxels of a grid path differ: no point is skipped)
                cur = centres[q][nxt[q]]
                if len(walks[q]) > 1 and not outside(cur, walks[q][-2]["planes"]):
                    walks[q].pop()
                if not walks[q] or outside(cur, walks[q][-1]["planes"]):
                    due.append(q)
                    break
                nxt[q] += 1
        if not due:
            return walks, failed, ms, rounds, made
        seeds = np.array([paths[q][nxt[q]] for q in due], np.int32)
        g = gen.polygon_generation(seeds, 1000, 0, fetch_clusters=False)
        ms += gen.last_ms()
        h = gen.hull_planes(RES, LOWER, batch=len(due), plane_capacity=16, vertex_capacity=16)
        ms += gen.last_ms()
        rounds += 1
        for i, q in enumerate(due):
            if g["rtn"][i] != cluster.CLUSTER_OK or h["rtn"][i] != cluster.HULL_OK:
                failed[q] = True
                continue
            v = g["vertex_idx"][i]
            walks[q].append(dict(planes=h["planes"][i], center=h["center"][i], seed=centres[q][nxt[q]],
                                 cube=[v[7], v[15], v[23], v[1], v[9], v[17]]))
            made += 1
            nxt[q] += 1


ms_b = []
for _ in range(WARM + CALLS):
    walks, failed, ms, rounds, made = lock_step()
    ms_b.append(ms)
gen.close()
completed = [q for q in range(NQ) if not failed[q]]
for q in completed:
    k = len(walks[q])
    assert cor["n_seg"][q] == k, q
    assert cor["planes"][q, :k].tobytes() == np.array([w["planes"] for w in walks[q]], np.float64).tobytes(), q
    assert cor["centers"][q, :k].tobytes() == np.array([w["center"] for w in walks[q]], np.float64).tobytes(), q
    assert cor["seeds"][q, :k].tobytes() == np.array([w["seed"] for w in walks[q]], np.float64).tobytes(), q
    assert cor["cube_idx"][q, :k].tolist() == [w["cube"] for w in walks[q]], q

med = lambda v: round(float(np.median(v[WARM:])), 4)
res = dict(queries=NQ, map=list(grid.shape), calls=CALLS, path_voxels_total=int(path_len.sum()), path_voxels_max=int(path_len.max()),
           grid_path_ms=med(ms_a), lock_step_ms=med(ms_b), lock_step_rounds=rounds, lock_step_polytopes_generated=made,
           lock_step_rows_completed=len(completed), cube_corridor_ms=med(ms_c), cube_corridor_ms_min=round(float(min(ms_c[WARM:])), 4),
           cube_corridor_ms_max=round(float(max(ms_c[WARM:])), 4), polytopes_kept=int(cor["n_seg"].sum()), polytopes_per_row_max=int(cor["n_seg"].max()),
           table_queries_per_cube_mean=round(float(queries.mean()), 1), table_queries_per_cube_max=int(queries.max()))
res["below_grid_path"] = bool(res["cube_corridor_ms"] < res["grid_path_ms"])
res["below_lock_step"] = bool(res["cube_corridor_ms"] < res["lock_step_ms"])
print("64 queries: grid paths %.3f ms; lock-step walk (1000, 0) %.3f ms in %d rounds (%d of %d rows completed, bit-equal); cube corridors %.3f ms "
      "(min %.3f, max %.3f) for %d path voxels, %d polytopes kept; table queries per cube: mean %.1f, max %d"
      % (res["grid_path_ms"], res["lock_step_ms"], rounds, len(completed), NQ, res["cube_corridor_ms"], res["cube_corridor_ms_min"],
         res["cube_corridor_ms_max"], res["path_voxels_total"], res["polytopes_kept"], res["table_queries_per_cube_mean"],
         res["table_queries_per_cube_max"]), flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"cube_corridor_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"cube_corridor_bench": res}))
