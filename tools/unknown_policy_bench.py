"""Time of one tracked scan (direct_cluster_map_integrate_scan with DIRECT_SCAN_TRACK_KNOWN) under the unknown policy
DIRECT_UNKNOWN_OCCUPIED beside the same scan under DIRECT_UNKNOWN_FREE, on the same inputs, in the same process, interleaved free,
occupied, free, occupied: the FREE scan's two runs are the yardstick and their difference is its spread.  Maps: the launch file's
(50 x 50 x 5 m at 0.15 m: 333 x 333 x 33 voxels) and 1024 x 1024 x 16; the origin mid-map, max_range 10 m,
problems.make_point_cloud clouds of 10^5 and 10^6 points in device memory, inflate (0, 0, 0) and (2, 2, 1).  Per call, from the
handle's own HIP events (DIRECT_CLUSTER_SCAN_TIMING=1): carve, mark, inflation and table rebuild; beside them
direct_cluster_last_ms; median of 20 calls after 3 warm-up calls.  Under OCCUPIED the inflation phase holds the dilation passes
(the x pass in its non-counting form) AND the close pass, so at inflate (0, 0, 0)
  close pass = inflate_ms(occupied) - inflate_ms(free),   yardstick = inflate_ms(free) = the x dilation pass of the same visit.
Two situations:
  static   the same scan again (CONTINUE): nothing changes, no group of the map is stored, the table stays
  changed  the map emptied by set_map (not timed), then the scan with RESET: the table is rebuilt
The device's grids, stats and policy counts are checked against the restatement of tests/unknown_policy_harness.py on a 4096-point
subset (equality) on the way.
usage: unknown_policy_bench.py [out.json]   (default profiles/unknown_policy_bench.json)"""
import json
import os
import sys

import numpy as np
import torch  # before the library is loaded: torch must initialise its HIP runtime first

sys.path.insert(0, ".")
os.environ["DIRECT_CLUSTER_SCAN_TIMING"] = "1"
from direct_amd import cluster, problems  # noqa: E402
from tests import evidence_harness as eh  # noqa: E402
from tests import unknown_policy_harness as uh  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "unknown_policy_bench.json")
CALLS, WARM = 20, 3
RES, RANGE = 0.15, 10.0
MAPS = (((333, 333, 33), np.array([-25.0, -25.0, 0.0]), np.array([0.07, -0.04, 2.45])),
        ((1024, 1024, 16), np.array([-76.8, -76.8, 0.0]), np.array([0.07, -0.04, 1.25])))
SMALL = dict(max_batch=1, cluster_capacity=64, candidate_capacity=64)
PHASES = ("carve", "mark", "inflate", "table")


def timed(gen, fn, before=None):
    ev, phase = [], []
    for _ in range(WARM + CALLS):
        if before is not None:
            before()
        torch.cuda.synchronize()
        fn()
        ev.append(gen.last_ms())
        phase.append(gen.scan_phase_ms())
    med = lambda v: round(float(np.median(v[WARM:])), 4)
    ph = np.array(phase[WARM:])
    out = dict(event_ms=med(ev), event_ms_min=round(float(min(ev[WARM:])), 4))
    out.update({name + "_ms": med(list(ph[:, k])) for k, name in enumerate(PHASES)})
    return out


rows, ok = [], True
for dims, lower, origin in MAPS:
    upper = lower + np.array(dims) * RES
    empty = np.zeros(dims, np.uint8)
    kw3 = dict(dims=dims, res=RES, lower=lower, upper=upper)
    handles = dict(free=cluster.ClusterGenerator(dims, **SMALL), occupied=cluster.ClusterGenerator(dims, **SMALL))
    handles["occupied"].set_unknown_policy("occupied")
    for n in (100000, 1000000):
        pts = problems.make_point_cloud(dims, RES, lower, seed=11, n_points=n)
        dev_pts = torch.from_numpy(pts).to("cuda:0")
        touched = eh.touch_grid(pts[:4096], origin, RANGE, dims, RES, lower, upper)
        for inflate in ((0, 0, 0), (2, 2, 1)):
            kw = dict(inflate=inflate, map_upper=upper, track_known=True)
            g = handles["occupied"]
            want = uh.restate_plain(pts[:4096], origin, RANGE, inflate, "reset", before=empty, touched=touched, **kw3)
            g.set_map(empty)
            st = g.integrate_scan(pts[:4096], origin, lower, RES, RANGE, mode="reset", **kw)
            equal = bool(np.array_equal(g.get_map(), want["map"]) and np.array_equal(g.open_map(), want["open"]) and
                         np.array_equal(g.scan_grid(), want["raw"]) and np.array_equal(g.known_grid(), want["known"]) and
                         [st[k] for k in cluster.SCAN_STATS] == want["stats"].tolist() and
                         g.unknown_policy() == dict(policy="occupied", closed=want["closed"], open_ones=want["open_ones"]))
            ok = ok and equal
            row = dict(map=list(dims), points=n, inflate=list(inflate), equal_to_restatement_on_4096_points=equal)

            def scan(name, mode):
                h = handles[name]
                return lambda: h.integrate_scan(dev_pts, origin, lower, RES, RANGE, mode=mode, **kw)

            for situation in ("static", "changed"):
                cell = {}
                for run in (1, 2):   # free, occupied, free, occupied
                    for name in ("free", "occupied"):
                        h = handles[name]
                        if situation == "static":
                            scan(name, "reset")()
                            last = scan(name, "continue")()
                            assert last["set"] + last["cleared"] == 0
                            cell["%s_%d" % (name, run)] = timed(h, scan(name, "continue"))
                        else:
                            cell["%s_%d" % (name, run)] = timed(h, scan(name, "reset"), before=lambda h=h: h.set_map(empty))
                cell["close_pass_ms"] = round(cell["occupied_1"]["inflate_ms"] - cell["free_1"]["inflate_ms"], 4)
                cell["free_spread_ms"] = round(abs(cell["free_1"]["event_ms"] - cell["free_2"]["event_ms"]), 4)
                row[situation] = cell
                f, o = cell["free_1"], cell["occupied_1"]
                print("%s %7d points, inflate %s, %-7s: free %.3f / %.3f ms (carve %.3f, mark %.3f, inflate %.3f, table %.3f); occupied %.3f / %.3f ms "
                      "(carve %.3f, mark %.3f, inflate %.3f, table %.3f); close pass %.3f ms"
                      % (dims, n, inflate, situation, f["event_ms"], cell["free_2"]["event_ms"], f["carve_ms"], f["mark_ms"], f["inflate_ms"],
                         f["table_ms"], o["event_ms"], cell["occupied_2"]["event_ms"], o["carve_ms"], o["mark_ms"], o["inflate_ms"], o["table_ms"],
                         cell["close_pass_ms"]), flush=True)
            rows.append(row)
    for h in handles.values():
        h.close()

res = dict(resolution=RES, max_range=RANGE, calls=CALLS, warmup=WARM, device=torch.cuda.get_device_name(0), equal_to_restatement=ok, rows=rows)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"unknown_policy_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"unknown_policy_bench": {"rows": len(rows), "equal_to_restatement": ok}}))
sys.exit(0 if ok else 1)
