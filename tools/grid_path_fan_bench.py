"""Time of direct_cluster_grid_path_fan_batch on the 200 x 200 x 40 map of tests/grid_path_harness.big_map(), in one process, timed by
direct_cluster_last_ms (HIP events), median of 20 calls after 3 warm-up calls each:
  (a) grid_paths (direct_cluster_grid_path_batch) on 64 pairs that share one start: what a caller had before the fan - the baseline;
  (b) the fan with that start and the same 64 goals;
  (c) the fan with that start and 4096 free goals drawn over the map;
  (d) (c) in clear mode with clearance_penalty_table(0.3, 4.0).
(b), (c) and (d) run twice, on a handle that refreshes the pruning bound before every round (the library's setting) and on one that
refreshes it once per eight rounds (DIRECT_CLUSTER_FAN_BOUND_EVERY=8, read when a handle is created); both must give the same bytes.
(b) must equal (a) byte for byte; of (c) and (d) every 64th goal is held against the pairwise call.  Every step that uses the device
runs under a time limit of its own (SIGALRM with the default action: the process ends there and starts nothing more).
usage: grid_path_fan_bench.py [out.json]   (default profiles/grid_path_fan_bench.json)"""
import contextlib
import json
import os
import signal
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402,F401  (before the library is loaded)
from direct_amd import cluster  # noqa: E402
from tests import grid_path_harness as gh  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "grid_path_fan_bench.json")
CALLS, WARM, NQ, NG, CAP = 20, 3, 64, 4096, 1024
TABLE = (0.3, 4.0)


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
                   fields=int(len(r["stats"])), rounds_max=int(r["stats"][:, 0].max()), tile_visits_total=int(r["stats"][:, 1].sum()),
                   goals=int(len(r["rtn"])), ok=int((r["rtn"] == cluster.GRID_PATH_OK).sum()),
                   path_voxels_mean=round(float(r["path_len"].mean()), 1))


def same(a, b, ia, ib, clear=False):
    """goals ia of result a and ib of result b: every per-goal byte"""
    keys = ("rtn", "path_len") + (("path_min_d2",) if clear else ())
    assert all(np.array_equal(a[k][ia], b[k][ib]) for k in keys)
    assert np.array_equal(a["path_cost"][ia].view(np.int64), b["path_cost"][ib].view(np.int64))
    assert all(np.array_equal(a["paths"][i], b["paths"][j]) for i, j in zip(ia, ib))
    assert not clear or all(np.array_equal(a["path_d2"][i], b["path_d2"][j]) for i, j in zip(ia, ib))


grid = gh.big_map()
starts, goals64 = gh.big_queries(grid, NQ)
start = starts[:1].copy()
free = np.argwhere(grid == 0)
goals4k = free[np.random.default_rng(17).integers(len(free), size=NG)].astype(np.int32)
pen = cluster.clearance_penalty_table(*TABLE)
every64 = np.arange(0, NG, NG // NQ)

with limit(120):
    gen = cluster.ClusterGenerator(grid.shape, max_batch=NQ, cluster_capacity=64, candidate_capacity=64)
    gen.set_map(grid)
    gen.build_distance_field()
with limit(180):
    pair, row_a = timed(gen, lambda: gen.grid_paths(np.repeat(start, NQ, axis=0), goals64, path_capacity=CAP))
    pair_c = gen.grid_paths(np.repeat(start, NQ, axis=0), goals4k[every64], path_capacity=CAP)
    pair_d = gen.grid_paths_clear(np.repeat(start, NQ, axis=0), goals4k[every64], 0, pen, path_capacity=CAP)
print("(a) 64 pairs, one start: %.3f ms (min %.3f, max %.3f), %d fields, up to %d rounds, %d tile visits"
      % (row_a["ms_median"], row_a["ms_min"], row_a["ms_max"], row_a["fields"], row_a["rounds_max"], row_a["tile_visits_total"]), flush=True)

rows = {}
for every in (1, 8):
    os.environ["DIRECT_CLUSTER_FAN_BOUND_EVERY"] = str(every)
    with limit(60):
        fan = cluster.ClusterGenerator(grid.shape, max_batch=1, cluster_capacity=64, candidate_capacity=64)
        fan.set_map(grid)
        fan.build_distance_field()
    with limit(300):
        b, row_b = timed(fan, lambda: fan.grid_paths_fan(start, goals64, path_capacity=CAP))
        c, row_c = timed(fan, lambda: fan.grid_paths_fan(start, goals4k, path_capacity=CAP))
        d, row_d = timed(fan, lambda: fan.grid_paths_fan(start, goals4k, penalty=pen, path_capacity=CAP))
        fan.close()
    same(b, pair, np.arange(NQ), np.arange(NQ))
    same(c, pair_c, every64, np.arange(NQ))
    same(d, pair_d, every64, np.arange(NQ), clear=True)
    if rows:
        for new, old, clear in ((b, rows[1]["results"][0], False), (c, rows[1]["results"][1], False), (d, rows[1]["results"][2], True)):
            same(new, old, np.arange(len(new["rtn"])), np.arange(len(new["rtn"])), clear)
    rows[every] = dict(b=row_b, c=row_c, d=row_d, results=(b, c, d))
    for name, row in (("b", row_b), ("c", row_c), ("d", row_d)):
        print("(%s) bound every %d: %d goals, %.3f ms (min %.3f, max %.3f), %d rounds, %d tile visits, %d OK"
              % (name, every, row["goals"], row["ms_median"], row["ms_min"], row["ms_max"], row["rounds_max"], row["tile_visits_total"], row["ok"]),
              flush=True)
del os.environ["DIRECT_CLUSTER_FAN_BOUND_EVERY"]
gen.close()

res = dict(map=list(grid.shape), calls=CALLS, warmup=WARM, path_capacity=CAP, device=torch.cuda.get_device_name(0), start=start[0].tolist(),
           table=dict(weight=TABLE[0], soft_radius_vox=TABLE[1]), equal_to_pairwise=dict(b=NQ, c=NQ, d=NQ),
           a_pairs_shared_start=row_a,
           bound_every_round={k: rows[1][k] for k in "bcd"}, bound_every_eight_rounds={k: rows[8][k] for k in "bcd"})
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"grid_path_fan_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"grid_path_fan_bench": dict(a_ms=row_a["ms_median"], every_round={k: rows[1][k]["ms_median"] for k in "bcd"},
                                              every_eight={k: rows[8][k]["ms_median"] for k in "bcd"})}))
