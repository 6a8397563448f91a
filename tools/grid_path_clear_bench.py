"""Time and effect of direct_cluster_grid_path_clear_batch for the 64 queries of tools/grid_path_bench.py on its 200 x 200 x 40 map,
in one process, timed by direct_cluster_last_ms (HIP events), median of 20 calls after 3 warm-up calls each:
  (a) the plain call, direct_cluster_grid_path_batch - the yardstick of (b), in the same run;
  (b) the new call with neutral parameters (min_d2 = 0, no table);
  (c) the new call with clearance_penalty_table(weight, r) for three (weight, r) pairs, with rounds and tile visits;
  (d) what the feature is for, on the chain: the paths of (a) and of every (c) through cube_corridors, direct_ddp_plan_batch
      (durations left to the library) and plan_clearance - polytopes per corridor, the median and the smallest cube edge, how
      many rows solve, the median and the minimum clearance of the solved plans, and the path length paid for it.
(b) and every (c) must equal the g++ build of the same arithmetic (tests/grid_path_clear_harness.py, the Dijkstra with goal
exit) bit for bit on all 64 queries; (b) must also equal (a).  Every step that uses the device runs under a time limit of its own
(SIGALRM with the default action: the process ends there and starts nothing more).
usage: grid_path_clear_bench.py [out.json]   (default profiles/grid_path_clear_bench.json)"""
import contextlib
import json
import os
import signal
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402,F401  (before the library is loaded)
from direct_amd import abi, cluster, solver  # noqa: E402
from tests import grid_path_clear_harness as ch  # noqa: E402
from tests import grid_path_harness as gh  # noqa: E402
from tests.real_corridor_lib import LOWER, RES  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "grid_path_clear_bench.json")
CALLS, WARM, NQ, CAP, SEG, P = 20, 3, 64, 4096, 96, 6
TABLES = ((0.3, 4.0), (1.0, 4.0), (1.0, 8.0))


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
    return r, dict(ms_median=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4), ms_max=round(float(max(ms)), 4),
                   rounds_max=int(r["stats"][:, 0].max()), rounds_mean=round(float(r["stats"][:, 0].mean()), 2),
                   tile_visits_total=int(r["stats"][:, 1].sum()), path_voxels_mean=round(float(r["path_len"].mean()), 1))


def equal_to_harness(dev, ref):
    assert np.array_equal(dev["rtn"], ref["rtn"]) and np.array_equal(dev["path_len"], ref["path_len"])
    assert np.array_equal(dev["path_cost"].view(np.int64), ref["path_cost"].view(np.int64))
    assert np.array_equal(dev["path_min_d2"], ref["path_min_d2"])
    assert all(np.array_equal(dev["paths"][q], ref["paths"][q]) and np.array_equal(dev["path_d2"][q], ref["path_d2"][q]) for q in range(NQ))


grid = gh.big_map()
starts, goals = gh.big_queries(grid, NQ)
harness = ch.build(tempfile.mkdtemp())
with limit(120):
    gen = cluster.ClusterGenerator(grid.shape, max_batch=NQ, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
    gen.build_distance_field()
    d2 = gen.distance_field()

with limit(120):
    plain, row_a = timed(gen, lambda: gen.grid_paths(starts, goals, path_capacity=CAP))
    neutral, row_b = timed(gen, lambda: gen.grid_paths_clear(starts, goals, path_capacity=CAP))
assert (plain["rtn"] == cluster.GRID_PATH_OK).all()
for k in ("rtn", "path_len"):
    assert np.array_equal(plain[k], neutral[k])
assert np.array_equal(plain["path_cost"].view(np.int64), neutral["path_cost"].view(np.int64))
assert all(np.array_equal(a, b) for a, b in zip(plain["paths"], neutral["paths"]))
equal_to_harness(neutral, ch.run(harness, grid, d2, starts, goals, 0, None, CAP, sides=("early",), fields=False)["early"])
row_b["inside_plain_spread"] = bool(row_a["ms_min"] <= row_b["ms_median"] <= row_a["ms_max"])
print("(a) plain %.3f ms (min %.3f, max %.3f), %d tile visits; (b) neutral %.3f ms (min %.3f, max %.3f), %d tile visits"
      % (row_a["ms_median"], row_a["ms_min"], row_a["ms_max"], row_a["tile_visits_total"], row_b["ms_median"], row_b["ms_min"], row_b["ms_max"],
         row_b["tile_visits_total"]), flush=True)


def chain(name, r):
    """(d): corridors, plans and clearances of one set of paths (host arrays in, one solver per set)"""
    xyz = np.zeros((NQ, CAP, 3), np.int32)
    for q in range(NQ):
        xyz[q, :len(r["paths"][q])] = r["paths"][q]
    with limit(60):
        cor = gen.cube_corridors(xyz, r["path_len"], LOWER, RES, seg_capacity=SEG, p_max=P)
    fit = (cor["rtn"] == cluster.CUBE_CORRIDOR_OK) & (cor["n_seg"] >= 1)
    idx = np.flatnonzero(fit)
    edges = np.concatenate([(cor["cube_idx"][q, :cor["n_seg"][q], 3:] - cor["cube_idx"][q, :cor["n_seg"][q], :3] + 1).min(axis=1) for q in idx])
    N = int(cor["n_seg"][idx].max())
    centre = lambda v: v.astype(np.float64) * RES + 0.5 * RES + LOWER
    x0, xd = np.zeros((len(idx), 9)), np.zeros((len(idx), 9))
    x0[:, :3] = centre(np.array([r["paths"][q][0] for q in idx]))
    xd[:, :3] = centre(np.array([r["paths"][q][-1] for q in idx]))
    hb = abi.HostBatch(cor["n_seg"][idx], x0, xd, np.zeros((len(idx), N)), cor["n_planes"][idx, :N], cor["planes"][idx, :N],
                       seeds=cor["seeds"][idx, :N]).without_T0()
    with limit(300):
        sol = solver.DdpSolver(len(idx), N, P, np.float64, device=0)
        _, plan = sol.plan(abi.phase0_params(), abi.phase1_params(), hb)
        sol.close()
    solved = plan.rtn >= 0
    with limit(60):
        clr = gen.plan_clearance(cor["n_seg"][idx], plan.T, LOWER, RES, poly=plan.poly)
    good = solved & (clr["status"] == 0) & np.isfinite(clr["clearance"])
    c = clr["clearance"][good]
    row = dict(paths=name, path_voxels_mean=round(float(r["path_len"].mean()), 1), path_cost_mean=round(float(r["path_cost"].mean()), 3),
               path_min_d2_median=float(np.median(r["path_min_d2"])), path_min_d2_min=int(r["path_min_d2"].min()),
               corridors=int(len(idx)), polytopes_per_corridor_mean=round(float(cor["n_seg"][idx].mean()), 2),
               polytopes_per_corridor_max=N, cube_edge_median_vox=float(np.median(edges)), cube_edge_min_vox=int(edges.min()),
               rows_solved=int(solved.sum()), plan_rtn={str(k): int((plan.rtn == k).sum()) for k in np.unique(plan.rtn)},
               clearance_rows=int(good.sum()), clearance_median_m=round(float(np.median(c)), 4) if len(c) else None,
               clearance_min_m=round(float(c.min()), 4) if len(c) else None)
    print("(d) %-10s %.1f voxels per path, min D2 on the path median %.0f; %.2f polytopes per corridor, cube edge median %.0f min %d voxels; "
          "%d of %d rows solve; clearance median %s m, min %s m"
          % (name, row["path_voxels_mean"], row["path_min_d2_median"], row["polytopes_per_corridor_mean"], row["cube_edge_median_vox"],
             row["cube_edge_min_vox"], row["rows_solved"], len(idx), row["clearance_median_m"], row["clearance_min_m"]), flush=True)
    return row


rows_c, rows_d = [], [chain("plain", dict(plain, path_min_d2=neutral["path_min_d2"]))]
for weight, r in TABLES:
    pen = cluster.clearance_penalty_table(weight, r)
    with limit(120):
        dev, row = timed(gen, lambda: gen.grid_paths_clear(starts, goals, 0, pen, path_capacity=CAP))
    equal_to_harness(dev, ch.run(harness, grid, d2, starts, goals, 0, pen, CAP, sides=("early",), fields=False)["early"])
    row.update(weight=weight, soft_radius_vox=r, table_entries=len(pen),
               paths_differing_from_plain=int(sum(not np.array_equal(dev["paths"][q], plain["paths"][q]) for q in range(NQ))))
    rows_c.append(row)
    print("(c) weight %.1f, radius %.0f: %.3f ms (min %.3f, max %.3f), up to %d rounds, %d tile visits, %d of %d paths differ from the plain ones"
          % (weight, r, row["ms_median"], row["ms_min"], row["ms_max"], row["rounds_max"], row["tile_visits_total"],
             row["paths_differing_from_plain"], NQ), flush=True)
    rows_d.append(chain("w%.1f_r%.0f" % (weight, r), dev))
gen.close()

res = dict(queries=NQ, map=list(grid.shape), calls=CALLS, warmup=WARM, device=torch.cuda.get_device_name(0), harness_equal_queries=NQ,
           plain=row_a, neutral=row_b, penalty=rows_c, chain=rows_d)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"grid_path_clear_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"grid_path_clear_bench": dict(plain_ms=row_a["ms_median"], neutral_ms=row_b["ms_median"],
                                                penalty_ms=[r["ms_median"] for r in rows_c])}))
