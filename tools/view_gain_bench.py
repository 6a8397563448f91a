"""Time of direct_cluster_view_gain_batch on the launch file's map (50 x 50 x 5 m at 0.15 m: 333 x 333 x 33 voxels): a
problems.make_point_cloud cloud of 10^5 points scanned once, tracked, from the origin mid-map at max_range 10 m; the candidates are
the frontier representatives of that scan (min_size 1) followed by its frontier voxels at an even stride of their linear index, as
many as the cell asks for - every one known, enterable and a legal goal.  Cells: n in (64, 1024) candidates x n_dirs in (1024, 8192)
directions (view_directions over a full turn, elevation +/- 0.5 rad) x range_vox in (12, 48), i.e. R = 14 and R = 50, the largest
box.  Per cell, from the handle's own HIP events, the median of 20 calls after 3 warm-up calls, host outputs, candidates and
directions resident in device memory:
  event_ms            the library as it ships: 1024 threads per workgroup (kViewThreads of direct_amd/csrc/view_gain.h)
  threads_256 / _512 / _1024   the same call on handles created with DIRECT_CLUSTER_VIEW_THREADS set
  cpu_ms              ONE thread of the g++ -O2 build of the same header on the same inputs (tests/view_gain_harness.py), the only
                      baseline there is; its outputs are compared with the device's on the way (equality)
  rays_per_s, visits_per_s   rays and visited voxels (repeats included, counted by the host program) per second of event_ms
usage: view_gain_bench.py [out.json]   (default profiles/view_gain_bench.json)"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch  # before the library is loaded: torch must initialise its HIP runtime first

sys.path.insert(0, ".")
from direct_amd import cluster, problems  # noqa: E402
from tests import view_gain_harness as vh  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "view_gain_bench.json")
CALLS, WARM = 20, 3
RES, RANGE, N_POINTS = 0.15, 10.0, 100000
DIMS, LOWER, ORIGIN = (333, 333, 33), np.array([-25.0, -25.0, 0.0]), np.array([0.07, -0.04, 2.45])
SMALL = dict(max_batch=1, cluster_capacity=64, candidate_capacity=64)
THREADS = (256, 512, 1024)
harness = vh.build(tempfile.mkdtemp(prefix="view_gain_bench_"))


def med(v):
    return round(float(np.median(v)), 4)


def timed(gen, fn):
    ev, wall = [], []
    for _ in range(WARM + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(gen.last_ms())
    ev, wall = ev[WARM:], wall[WARM:]
    return r, dict(event_ms=med(ev), event_ms_min=round(float(min(ev)), 4), event_ms_max=round(float(max(ev)), 4), wall_ms=med(wall))


def handle(grid, known, threads=None):
    if threads is None:
        os.environ.pop("DIRECT_CLUSTER_VIEW_THREADS", None)
    else:
        os.environ["DIRECT_CLUSTER_VIEW_THREADS"] = str(threads)   # read when the handle is created
    g = cluster.ClusterGenerator(DIMS, **SMALL)
    os.environ.pop("DIRECT_CLUSTER_VIEW_THREADS", None)
    g.set_map(grid)
    g.set_known(known)
    return g


upper = LOWER + np.array(DIMS) * RES
pts = problems.make_point_cloud(DIMS, RES, LOWER, seed=11, n_points=N_POINTS)
first = cluster.ClusterGenerator(DIMS, **SMALL)
first.integrate_scan(pts, ORIGIN, LOWER, RES, RANGE, mode="reset", map_upper=upper, track_known=True)
grid, known = first.get_map(), first.known_grid()
front = first.frontiers(min_size=1, capacity=65536, voxel_labels=True)
first.close()
on_front = np.flatnonzero(front["voxel_label"].reshape(-1) >= 0)
scene = dict(occupied=int(grid.sum()), known=int(known.sum()), frontier_voxels=int(len(on_front)), representatives=int(len(front["rep"])))
print("scene: %s" % scene, flush=True)


def candidates(n):
    rep = front["rep"][:n]
    idx = on_front[np.linspace(0, len(on_front) - 1, n - len(rep)).astype(np.int64)] if n > len(rep) else np.zeros(0, np.int64)
    vox = np.stack([idx // (DIMS[1] * DIMS[2]), (idx // DIMS[2]) % DIMS[1], idx % DIMS[2]], axis=1)
    return np.ascontiguousarray(np.concatenate([rep, vox.astype(np.int32)]), np.int32)


gens = dict(shipped=handle(grid, known))
for t in THREADS:
    gens[t] = handle(grid, known, t)
rows, ok = [], True
for n in (64, 1024):
    cand = candidates(n)
    dev_cand = torch.from_numpy(cand).to("cuda:0")
    for n_dirs, (n_az, n_el) in ((1024, (64, 16)), (8192, (256, 32))):
        dirs = cluster.view_directions(n_az, n_el, -0.5, 0.5)
        dev_dirs = torch.from_numpy(dirs).to("cuda:0")
        for range_vox in (12.0, 48.0):
            cpu = vh.run(harness, grid, known, cand, dirs, range_vox)
            got, row = timed(gens["shipped"], lambda: gens["shipped"].view_gain(dev_cand, dev_dirs, range_vox))
            same = all(np.array_equal(got[k], cpu[k]) for k in vh.KEYS)
            ok = ok and same
            rays = n * n_dirs
            row.update(n=n, n_dirs=n_dirs, range_vox=range_vox, box_half=vh.box_half(range_vox), equal_to_host_program=same,
                       cpu_ms=round(cpu["ms"], 3), rays=rays, visits=cpu["visits"], seen=int(cpu["seen"].sum()), gain=int(cpu["gain"].sum()),
                       rays_per_s=round(rays / (row["event_ms"] * 1e-3)), visits_per_s=round(cpu["visits"] / (row["event_ms"] * 1e-3)),
                       cpu_over_device=round(cpu["ms"] / row["event_ms"], 1))
            for t in THREADS:
                alt, tr = timed(gens[t], lambda: gens[t].view_gain(dev_cand, dev_dirs, range_vox))
                ok = ok and all(np.array_equal(alt[k], cpu[k]) for k in vh.KEYS)
                row["threads_%d" % t] = tr["event_ms"]
            rows.append(row)
            print("n %4d, n_dirs %4d, range_vox %2d: %.3f ms (min %.3f, max %.3f; 256 / 512 / 1024 threads %.3f / %.3f / %.3f), wall %.3f ms; "
                  "one CPU thread %.1f ms (%.0fx); %.3g rays/s, %.3g visits/s; equal %s"
                  % (n, n_dirs, range_vox, row["event_ms"], row["event_ms_min"], row["event_ms_max"], row["threads_256"], row["threads_512"],
                     row["threads_1024"], row["wall_ms"], row["cpu_ms"], row["cpu_over_device"], row["rays_per_s"], row["visits_per_s"], same),
                  flush=True)
for g in gens.values():
    g.close()

res = dict(map="launch_file_333x333x33", resolution=RES, scan_max_range=RANGE, points=N_POINTS, calls=CALLS, warmup=WARM,
           device=torch.cuda.get_device_name(0), scene=scene, equal_to_host_program=ok, rows=rows)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"view_gain_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"view_gain_bench": {"rows": len(rows), "equal_to_host_program": ok}}))
sys.exit(0 if ok else 1)
