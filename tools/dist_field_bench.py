"""Time of direct_cluster_distance_field and direct_cluster_plan_clearance_batch, median of 20 calls after 3 warm-up calls.
usage: dist_field_bench.py [out.json] [B] [N]   (default profiles/dist_field_bench.json, B = 4096, N = 100)
Field:     the launch file's map (50 x 50 x 5 m at 0.15 m: 333 x 333 x 33 voxels), built from problems.make_point_cloud clouds by
           direct_cluster_map_from_cloud: "empty" (no points), "sparse" (10^4 points, margin 0) and "dense" (10^6 points, margin
           0.25), each uncapped and with cap_vox = 8.  direct_cluster_last_ms (HIP events: the three passes) and wall clock around
           the call; the same header (dist_field_math.h) on one host thread, g++ -O2, best of 3; equality of the two fields.
Clearance: the plans and the map of tools/plan_check_bench.py (B x N config-3 corridors solved on the device, float storage;
           1024 x 1024 x 16 voxels of 0.7 m, cluttered), at depth 6 and 8, against check_plans on the same plans in the same run,
           and the field of that map."""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (before the library: torch initialises its HIP runtime first)

from direct_amd import abi, cluster, problems, solver  # noqa: E402
from tests import dist_field_harness as dh  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "dist_field_bench.json")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
N = int(sys.argv[3]) if len(sys.argv) > 3 else 100
CALLS, WARM = 20, 3
dev = torch.device("cuda", 0)
harness = dh.build(tempfile.mkdtemp(prefix="dist_field_bench_"))


def timed(gen, fn):
    ev, wall = [], []
    for _ in range(WARM + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(gen.last_ms())
    med = lambda v: round(float(np.median(v[WARM:])), 4)
    return dict(event_ms=med(ev), event_ms_min=round(float(min(ev[WARM:])), 4), event_ms_max=round(float(max(ev[WARM:])), 4), wall_ms=med(wall))


# ---- the field on the launch file's map ----------------------------------------------------------------------------------
RES, LOWER = 0.15, np.array([-25.0, -25.0, 0.0])
DIMS = tuple(int(v * (1.0 / RES)) for v in (50.0, 50.0, 5.0))
assert DIMS == (333, 333, 33)
gen = cluster.ClusterGenerator(DIMS, max_batch=1, cluster_capacity=64, candidate_capacity=64)
field_rows = []
for name, n_points, margin in (("empty", 0, 0.0), ("sparse", 10000, 0.0), ("dense", 1000000, 0.25)):
    pts = problems.make_point_cloud(DIMS, RES, LOWER, seed=11, n_points=n_points) if n_points else np.zeros((0, 3), np.float32)
    gen.set_map_from_cloud(pts, LOWER, RES, margin)
    grid = gen.get_map()
    for cap in (0, 8):
        want, wstats, host_ms = dh.run_field(harness, grid, cap, reps=3)
        stats = gen.build_distance_field(cap)
        assert np.array_equal(gen.distance_field(), want) and stats == wstats, (name, cap)
        t = timed(gen, lambda: gen.build_distance_field(cap))
        row = dict(case=name, cap_vox=cap, occupied=int(grid.sum()), below_cap=stats["below_cap"], max_d2=stats["max_d2"], device=t,
                   host_one_thread_ms=round(host_ms, 3), speedup_events=round(host_ms / t["event_ms"], 1))
        field_rows.append(row)
        print("%-6s cap %d: %8d occupied, max D2 %d; device %.3f ms by events (min %.3f, max %.3f), %.3f ms wall; one host thread %.1f ms"
              % (name, cap, row["occupied"], stats["max_d2"], t["event_ms"], t["event_ms_min"], t["event_ms_max"], t["wall_ms"], host_ms), flush=True)
gen.close()

# ---- the clearance on the plan check's plans -----------------------------------------------------------------------------
PDIMS, PRES = (1024, 1024, 16), 0.7
PLOWER = np.array([-0.5 * PDIMS[0] * PRES, -0.5 * PDIMS[1] * PRES, -4.0])
batch = problems.make_batch("corridor", B, N, seed=1000)
s = solver.DdpSolver(B, N, batch.p_max, np.float64)
_, plan = s.plan(abi.phase0_params(), abi.phase1_params(iter_max=20, fixed_iters=1), batch)
s.close()
host = dict(n_seg=np.ascontiguousarray(batch.n_seg, np.int32), T=np.ascontiguousarray(plan.T, np.float32),
            poly=np.ascontiguousarray(plan.poly, np.float32))
dv = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
clutter, _ = problems.make_voxel_map(PDIMS, seed=7, n_pillars=1000, n_boxes=400, n_rings=100)
gen = cluster.ClusterGenerator(PDIMS, max_batch=1, cluster_capacity=64, candidate_capacity=64)
gen.set_map(clutter)
want, wstats, host_ms = dh.run_field(harness, clutter, 0, reps=1)
stats = gen.build_distance_field()
d2 = gen.distance_field()
assert np.array_equal(d2, want) and stats == wstats
t = timed(gen, lambda: gen.build_distance_field())
big = dict(map=list(PDIMS), occupied=int(clutter.sum()), max_d2=stats["max_d2"], device=t, host_one_thread_ms=round(host_ms, 3))
print("plan map %s: field %.3f ms by events, %.3f ms wall; one host thread %.1f ms" % (PDIMS, t["event_ms"], t["wall_ms"], host_ms), flush=True)
clear_rows = []
sample = np.linspace(0, B - 1, min(16, B)).astype(int)
for D in (6, 8):
    kw = dict(map_lower=PLOWER, resolution=PRES, depth=D)
    out = gen.plan_clearance(dv["n_seg"], dv["T"], poly=dv["poly"], radius=0.5, **kw)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ref = dh.run_clear(harness, {k: v[sample] for k, v in host.items()}, d2, D, 0.5, lower=PLOWER, res=PRES)
    dh.assert_same({k: v[sample] for k, v in got.items()}, ref, "D%d" % D)          # equality with the header on the host
    tc = timed(gen, lambda: gen.plan_clearance(dv["n_seg"], dv["T"], poly=dv["poly"], radius=0.5, **kw))
    tk = timed(gen, lambda: gen.check_plans(dv["n_seg"], dv["T"], poly=dv["poly"], **kw))
    leaves = int(host["n_seg"].sum()) << D
    ok = got["status"] == 0
    fin = ok & np.isfinite(got["clearance"])
    row = dict(depth=D, rows=B, segments=N, leaves=leaves, clearance=tc, check_plans=tk, clearance_over_check=round(tc["event_ms"] / tk["event_ms"], 2),
               leaves_per_us=round(leaves / (tc["event_ms"] * 1e3), 1), valid_rows=int(ok.sum()), below_radius_rows=int((got["verdict"] == 1).sum()),
               clearance_median_m=round(float(np.median(got["clearance"][fin])), 3), harness_equal_rows=int(len(sample)))
    clear_rows.append(row)
    print("D=%d: clearance %.3f ms by events (min %.3f, max %.3f), %.3f ms wall, %.0f leaves per us; check_plans %.3f ms; %d of %d rows below 0.5 m, "
          "median clearance %.2f m" % (D, tc["event_ms"], tc["event_ms_min"], tc["event_ms_max"], tc["wall_ms"], row["leaves_per_us"], tk["event_ms"],
                                       row["below_radius_rows"], row["valid_rows"], row["clearance_median_m"]), flush=True)
gen.close()

res = dict(calls=CALLS, warmup=WARM, device=torch.cuda.get_device_name(0), launch_map=list(DIMS), field=field_rows, plan_map_field=big,
           clearance=clear_rows)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"dist_field_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"dist_field_bench": dict(field=[(r["case"], r["cap_vox"], r["device"]["event_ms"]) for r in field_rows],
                                           clearance=[(r["depth"], r["clearance"]["event_ms"], r["check_plans"]["event_ms"]) for r in clear_rows])}))
