"""Time of building the resident voxel map from a point cloud on the launch file's map (50 x 50 x 5 m at 0.15 m: 333 x 333 x 33
voxels), for problems.make_point_cloud clouds of 10^5 and 10^6 points at margins 0.0, 0.25 and 0.45.  Two routes, same machine,
same run:
  host    what a caller had to do before: the reference's loop nest on one host thread (the g++ -O2 program of
          tests/map_cloud_harness.py, best of 3), then direct_cluster_set_map of the finished grid from host memory (wall clock)
  device  direct_cluster_map_from_cloud with the cloud in host memory and in device memory: direct_cluster_last_ms (HIP events:
          clear + rasterise + summed-area table) and wall clock (with the copy of the cloud), median of 20 calls after 3 warm-up
          calls
and, from a call with no points, what the clear and the summed-area rebuild alone cost: the part that does not shrink with the
cloud.  Whether bucketing the points by x-slab in front of the kernel could pay is measured too: the same call on the cloud
sorted by x beforehand (what a bucketing pass would hand the kernel, at no cost) - the kernel time it saves is the most such a
pass could earn before its own cost.  The device's map is checked against the host program's on the way (bit equality).
usage: map_cloud_bench.py [out.json]   (default profiles/map_cloud_bench.json)"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch  # before the library is loaded: torch must initialise its HIP runtime first

sys.path.insert(0, ".")
from direct_amd import cluster, problems  # noqa: E402
from tests import map_cloud_harness as mh  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "map_cloud_bench.json")
CALLS, WARM = 20, 3
RES, LOWER, UPPER = 0.15, np.array([-25.0, -25.0, 0.0]), np.array([25.0, 25.0, 5.0])
DIMS = tuple(int(v * (1.0 / RES)) for v in (50.0, 50.0, 5.0))  # TRP:1202-1204
assert DIMS == (333, 333, 33)

harness = mh.build(tempfile.mkdtemp())
gen = cluster.ClusterGenerator(DIMS, max_batch=1, cluster_capacity=64, candidate_capacity=64)


def timed(fn):
    ev, wall = [], []
    for _ in range(WARM + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(gen.last_ms())
    med = lambda v: round(float(np.median(v[WARM:])), 4)
    return dict(event_ms=med(ev), event_ms_min=round(float(min(ev[WARM:])), 4), wall_ms=med(wall))


rows = []
empty = timed(lambda: gen.set_map_from_cloud(np.zeros((0, 3), np.float32), LOWER, RES, 0.0, map_upper=UPPER))
print("no points (clear + summed-area table): %.3f ms by events, %.3f ms wall" % (empty["event_ms"], empty["wall_ms"]), flush=True)
for n in (100000, 1000000):
    pts = problems.make_point_cloud(DIMS, RES, LOWER, seed=11, n_points=n)
    dev_pts = torch.from_numpy(pts).to("cuda:0")
    dev_sorted = torch.from_numpy(np.ascontiguousarray(pts[np.argsort(pts[:, 0], kind="stable")])).to("cuda:0")
    for margin in (0.0, 0.25, 0.45):
        for bname, border in (("clamp", mh.CLAMP), ("drop", mh.DROP)):
            want, wstats, host_ms = mh.run(harness, pts, margin, border, DIMS, RES, LOWER, UPPER, reps=3)
            wall = []
            for _ in range(WARM + 5):
                t0 = time.perf_counter()
                gen.set_map(want)
                wall.append((time.perf_counter() - t0) * 1e3)
            set_map_ms = float(np.median(wall[WARM:]))
            st = gen.set_map_from_cloud(pts, LOWER, RES, margin, map_upper=UPPER, border=bname)
            assert np.array_equal(gen.get_map(), want) and [st["points"], st["skipped_nonfinite"], st["dropped"], st["occupied"]] == wstats.tolist()
            host = timed(lambda: gen.set_map_from_cloud(pts, LOWER, RES, margin, map_upper=UPPER, border=bname))
            dev = timed(lambda: gen.set_map_from_cloud(dev_pts, LOWER, RES, margin, map_upper=UPPER, border=bname))
            assert np.array_equal(gen.get_map(), want)
            srt = timed(lambda: gen.set_map_from_cloud(dev_sorted, LOWER, RES, margin, map_upper=UPPER, border=bname))
            assert np.array_equal(gen.get_map(), want)
            s, sz = mh.steps(margin, RES)
            row = dict(points=n, margin=margin, border=bname, steps=[s, sz], writes_per_point=(2 * s + 1) ** 2 * (2 * sz + 1),
                       occupied=int(wstats[3]), dropped=int(wstats[2]),
                       host_loop_ms=round(host_ms, 3), host_set_map_ms=round(set_map_ms, 3), host_route_ms=round(host_ms + set_map_ms, 3),
                       device_from_host=host, device_from_device=dev,
                       device_from_device_sorted_by_x_event_ms=srt["event_ms"],
                       table_share_of_event_ms=round(empty["event_ms"] / dev["event_ms"], 3),
                       speedup_wall_from_host=round((host_ms + set_map_ms) / host["wall_ms"], 1),
                       speedup_wall_from_device=round((host_ms + set_map_ms) / dev["wall_ms"], 1))
            rows.append(row)
            print("%7d points, margin %.2f (%3d writes/point), %-5s: host loop %.1f ms + set_map %.2f ms; device %.3f ms by events "
                  "(%.0f %% of it clear + table), wall %.3f ms from host memory, %.3f ms from device memory"
                  % (n, margin, row["writes_per_point"], bname, host_ms, set_map_ms, dev["event_ms"], 100 * row["table_share_of_event_ms"],
                     host["wall_ms"], dev["wall_ms"]), flush=True)
gen.close()

res = dict(map=list(DIMS), resolution=RES, calls=CALLS, warmup=WARM, device=torch.cuda.get_device_name(0), no_points=empty, rows=rows)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"map_cloud_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"map_cloud_bench": {"no_points": empty, "rows": len(rows)}}))
