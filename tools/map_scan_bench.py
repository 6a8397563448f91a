"""Time of folding one sensor scan into the resident map (direct_cluster_map_integrate_scan) on the launch file's map (50 x 50 x 5 m
at 0.15 m: 333 x 333 x 33 voxels), the origin mid-map, max_range 10 m, problems.make_point_cloud clouds of 10^5 and 10^6 points
in device memory, inflate (0, 0, 0) and (2, 2, 1).  Per call, from the handle's own HIP events (DIRECT_CLUSTER_SCAN_TIMING=1):
the carve, the mark, the inflation and the table rebuild; beside them direct_cluster_last_ms and the wall clock; median of 20 calls
after 3 warm-up calls.  Three situations:
  static   the same scan again (CONTINUE): nothing changes, no table is rebuilt - the 10 Hz node in a room that stands still
  changed  the map emptied by set_map (not timed), then the scan with RESET: every return is new, the table is rebuilt
  full     a map of ones adopted: every voxel a ray passes holds a 1, so every store of the carve lands
Both store variants of the carve are timed, on two handles of the same process: "test" loads the byte and stores only where it
is not 0 yet, "plain" stores unconditionally (DIRECT_CLUSTER_SCAN_STORE).  Yardsticks of the same run: direct_cluster_map_from_cloud
(ADD, margin 0) on the same cloud, and the g++ -O2 build of the same header on one host thread (tests/map_scan_harness.py).  The
device's grids and stats are checked against that program's on a 4096-point subset (equality) on the way.
usage: map_scan_bench.py [out.json]   (default profiles/map_scan_bench.json)"""
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
from tests import map_scan_harness as sh  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "map_scan_bench.json")
CALLS, WARM = 20, 3
RES, LOWER, UPPER = 0.15, np.array([-25.0, -25.0, 0.0]), np.array([25.0, 25.0, 5.0])
DIMS = (333, 333, 33)
ORIGIN, RANGE = np.array([0.07, -0.04, 2.45]), 10.0
SMALL = dict(max_batch=1, cluster_capacity=64, candidate_capacity=64)

harness = sh.build(tempfile.mkdtemp())
gens = {}
for variant in ("test", "plain"):
    os.environ["DIRECT_CLUSTER_SCAN_STORE"] = variant
    gens[variant] = cluster.ClusterGenerator(DIMS, **SMALL)
EMPTY, FULL = np.zeros(DIMS, np.uint8), np.ones(DIMS, np.uint8)


def timed(gen, fn, before=None, phases=True):
    ev, wall, phase = [], [], []
    for _ in range(WARM + CALLS):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(gen.last_ms())
        phase.append(gen.scan_phase_ms() if phases else [0.0] * 4)
    med = lambda v: round(float(np.median(v[WARM:])), 4)
    ph = np.array(phase[WARM:])
    out = dict(event_ms=med(ev), event_ms_min=round(float(min(ev[WARM:])), 4), wall_ms=med(wall))
    if phases:
        out.update(carve_ms=med(list(ph[:, 0])), mark_ms=med(list(ph[:, 1])), inflate_ms=med(list(ph[:, 2])), table_ms=med(list(ph[:, 3])))
    return out


def same_as_harness(gen, pts, inflate):
    raw, new, wstats, _ = sh.run(harness, pts, ORIGIN, RANGE, inflate, dims=DIMS, res=RES, lower=LOWER, upper=UPPER)
    gen.set_map(EMPTY)
    st = gen.integrate_scan(pts, ORIGIN, LOWER, RES, RANGE, inflate=inflate, mode="reset", map_upper=UPPER)
    return bool(np.array_equal(gen.scan_grid(), raw) and np.array_equal(gen.get_map(), new) and [st[k] for k in sh.STATS] == wstats.tolist())


rows = []
for n in (100000, 1000000):
    pts = problems.make_point_cloud(DIMS, RES, LOWER, seed=11, n_points=n)
    dev_pts = torch.from_numpy(pts).to("cuda:0")
    _, _, wstats, host_ms = sh.run(harness, pts, ORIGIN, RANGE, (0, 0, 0), dims=DIMS, res=RES, lower=LOWER, upper=UPPER)
    g0 = gens["test"]
    g0.set_map(EMPTY)

    def add():
        g0.set_map_from_cloud(dev_pts, LOWER, RES, 0.0, map_upper=UPPER, add=True)
    from_cloud = timed(g0, add, phases=False)
    for inflate in ((0, 0, 0), (2, 2, 1)):
        row = dict(points=n, inflate=list(inflate), truncated=int(wstats[2]), outside=int(wstats[3]), raw_occupied=int(wstats[4]),
                   host_one_thread_ms=round(host_ms, 2), map_from_cloud_add_margin0=from_cloud)
        for variant, gen in gens.items():
            row["equal_to_host_program_on_4096_points_" + variant] = same_as_harness(gen, pts[:4096], inflate)

            def scan(mode="continue"):
                return gen.integrate_scan(dev_pts, ORIGIN, LOWER, RES, RANGE, inflate=inflate, mode=mode, map_upper=UPPER)
            scan("reset")
            static = timed(gen, scan)

            def scan():  # noqa: F811
                return gen.integrate_scan(dev_pts, ORIGIN, LOWER, RES, RANGE, inflate=inflate, mode="reset", map_upper=UPPER)
            changed = timed(gen, scan, before=lambda: gen.set_map(EMPTY))

            def scan():  # noqa: F811
                return gen.integrate_scan(dev_pts, ORIGIN, LOWER, RES, RANGE, inflate=inflate, mode="adopt", map_upper=UPPER)
            full = timed(gen, scan, before=lambda: gen.set_map(FULL))
            row[variant] = dict(static=static, changed=changed, full=full)
            print("%7d points, inflate %s, %-5s: static %.3f ms (carve %.3f, mark %.3f, inflate %.3f, table %.3f); changed %.3f ms "
                  "(carve %.3f, table %.3f); full grid %.3f ms (carve %.3f); wall %.3f ms; map_from_cloud ADD %.3f ms; host %.1f ms"
                  % (n, inflate, variant, static["event_ms"], static["carve_ms"], static["mark_ms"], static["inflate_ms"], static["table_ms"],
                     changed["event_ms"], changed["carve_ms"], changed["table_ms"], full["event_ms"], full["carve_ms"], static["wall_ms"],
                     from_cloud["event_ms"], host_ms), flush=True)
        rows.append(row)
for gen in gens.values():
    gen.close()

ok = all(v for r in rows for k, v in r.items() if k.startswith("equal_"))
res = dict(map=list(DIMS), resolution=RES, origin=list(ORIGIN), max_range=RANGE, calls=CALLS, warmup=WARM, device=torch.cuda.get_device_name(0),
           equal_to_host_program=ok, rows=rows)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"map_scan_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"map_scan_bench": {"rows": len(rows), "equal_to_host_program": ok}}))
sys.exit(0 if ok else 1)
