"""Time of the tracked scan and of the frontier call (direct_cluster_map_integrate_scan with DIRECT_SCAN_TRACK_KNOWN,
direct_cluster_frontier) on the launch file's map (50 x 50 x 5 m at 0.15 m: 333 x 333 x 33 voxels) and on the 16.8 M-voxel map of
the component bench (1024 x 1024 x 16), the origin mid-map, max_range 10 m, a problems.make_point_cloud cloud of 10^5 points in
device memory, inflate (0, 0, 0).  From the handles' own HIP events (DIRECT_CLUSTER_SCAN_TIMING=1), median of 20 calls after 3
warm-up calls:
  scan      the same scan again (CONTINUE: nothing changes, no table is rebuilt) and the scan with RESET on an emptied map, tracked
            on one handle and untracked on a second handle with the same settings: event time, carve and mark
  frontier  the call after the tracked scan, min_size 1 and 5, capacity 1024 and 65536, host outputs: event time and its phases
            (mask, labelling, compaction, goals), and the counts it returned
On a 4096-point subset of the launch map's cloud the device's known grid and frontier outputs are checked against the g++ build of
the same headers (tests/frontier_harness.py) on the way (equality).
usage: frontier_bench.py [out.json]   (default profiles/frontier_bench.json)"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch  # before the library is loaded: torch must initialise its HIP runtime first

sys.path.insert(0, ".")
os.environ["DIRECT_CLUSTER_SCAN_TIMING"] = "1"
from direct_amd import cluster, problems  # noqa: E402
from tests import frontier_harness as fr  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "frontier_bench.json")
CALLS, WARM = 20, 3
RES, RANGE, N = 0.15, 10.0, 100000
SMALL = dict(max_batch=1, cluster_capacity=64, candidate_capacity=64)
MAPS = (("launch_file_333x333x33", (333, 333, 33), np.array([-25.0, -25.0, 0.0]), np.array([0.07, -0.04, 2.45])),
        ("components_bench_1024x1024x16", (1024, 1024, 16), np.array([-76.8, -76.8, 0.0]), np.array([0.07, -0.04, 1.21])))
harness = fr.build(tempfile.mkdtemp(prefix="frontier_bench_"))


def med(v):
    return round(float(np.median(v)), 4)


def timed(gen, fn, phase, before=None):
    ev, wall, ph = [], [], []
    for _ in range(WARM + CALLS):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(gen.last_ms())
        ph.append(phase())
    ev, wall, ph = ev[WARM:], wall[WARM:], np.array(ph[WARM:])
    return r, dict(event_ms=med(ev), event_ms_min=round(float(min(ev)), 4), event_ms_max=round(float(max(ev)), 4), wall_ms=med(wall)), ph


rows, ok = [], True
for name, dims, lower, origin in MAPS:
    upper = lower + np.array(dims) * RES
    pts = problems.make_point_cloud(dims, RES, lower, seed=11, n_points=N)
    dev_pts = torch.from_numpy(pts).to("cuda:0")
    tracked, plain = cluster.ClusterGenerator(dims, **SMALL), cluster.ClusterGenerator(dims, **SMALL)
    empty = np.zeros(dims, np.uint8)
    row = dict(map=name, voxels=int(np.prod(dims)), points=N)
    if name.startswith("launch"):   # equality with the host program on a subset, before anything is timed
        sub = pts[:4096]
        tracked.integrate_scan(sub, origin, lower, RES, RANGE, mode="reset", map_upper=upper, track_known=True)
        want = fr.run_scan(harness, sub, origin, RANGE, mode=fr.RESET, dims=dims, res=RES, lower=lower, upper=upper)
        known, grid = tracked.known_grid(), tracked.get_map()
        same = bool(np.array_equal(known, want["known"]) and np.array_equal(tracked.scan_grid(), want["raw"]))
        got = tracked.frontiers(min_size=2, capacity=4096, voxel_labels=True)
        ref = fr.run_frontier(harness, grid, known, min_size=2, capacity=4096)
        same = same and all(np.array_equal(got[k], ref[k]) for k in ("label", "size", "centroid", "rep", "voxel_label"))
        same = same and [got["stats"][k] for k in fr.STATS] == ref["stats"].tolist()
        row["equal_to_host_program_on_4096_points"] = same
        ok = ok and same
    for label, gen, track in (("tracked", tracked, True), ("untracked", plain, False)):
        def scan(mode="continue"):
            return gen.integrate_scan(dev_pts, origin, lower, RES, RANGE, mode=mode, map_upper=upper, track_known=track)
        scan("reset")
        _, static, ph = timed(gen, scan, gen.scan_phase_ms)
        static.update(carve_ms=med(ph[:, 0]), mark_ms=med(ph[:, 1]))
        _, changed, ph = timed(gen, lambda: scan("reset"), gen.scan_phase_ms, before=lambda: gen.set_map(empty))
        changed.update(carve_ms=med(ph[:, 0]), mark_ms=med(ph[:, 1]), table_ms=med(ph[:, 3]))
        row[label] = dict(static=static, changed=changed)
        print("%s %-9s scan: static %.3f ms (min %.3f, max %.3f; carve %.3f, mark %.3f); changed %.3f ms (carve %.3f)"
              % (name, label, static["event_ms"], static["event_ms_min"], static["event_ms_max"], static["carve_ms"], static["mark_ms"],
                 changed["event_ms"], changed["carve_ms"]), flush=True)
    tracked.integrate_scan(dev_pts, origin, lower, RES, RANGE, mode="reset", map_upper=upper, track_known=True)
    row["frontier"] = []
    for min_size, cap in ((1, 1024), (5, 1024), (1, 65536)):
        r, t, ph = timed(tracked, lambda: tracked.frontiers(min_size=min_size, capacity=cap), tracked.frontier_phase_ms)
        t.update(min_size=min_size, capacity=cap, mask_ms=med(ph[:, 0]), labelling_ms=med(ph[:, 1]), compaction_ms=med(ph[:, 2]),
                 goals_ms=med(ph[:, 3]), stats=r["stats"])
        row["frontier"].append(t)
        print("%s frontier min_size %d capacity %d: %.3f ms (mask %.3f, labelling %.3f, compaction %.3f, goals %.3f) wall %.3f ms; %s"
              % (name, min_size, cap, t["event_ms"], t["mask_ms"], t["labelling_ms"], t["compaction_ms"], t["goals_ms"], t["wall_ms"],
                 r["stats"]), flush=True)
    rows.append(row)
    tracked.close()
    plain.close()

res = dict(resolution=RES, max_range=RANGE, calls=CALLS, warmup=WARM, device=torch.cuda.get_device_name(0), equal_to_host_program=ok, rows=rows)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"frontier_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"frontier_bench": {"rows": len(rows), "equal_to_host_program": ok}}))
sys.exit(0 if ok else 1)
