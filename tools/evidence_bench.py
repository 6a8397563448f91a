"""Time of folding one sensor scan into the resident evidence grid (direct_cluster_map_integrate_scan_evidence) beside the plain
tracked scan (direct_cluster_map_integrate_scan with DIRECT_SCAN_TRACK_KNOWN) on the same inputs, in the same process, interleaved
plain, evidence, plain, evidence: the plain scan's two runs are the yardstick and their difference is its spread.  Maps: the launch
file's (50 x 50 x 5 m at 0.15 m: 333 x 333 x 33 voxels) and 1024 x 1024 x 16; the origin mid-map, max_range 10 m,
problems.make_point_cloud clouds of 10^5 and 10^6 points in device memory, inflate (0, 0, 0) and (2, 2, 1), both tracked.  Per call,
from the handle's own HIP events (DIRECT_CLUSTER_SCAN_TIMING=1): touch, hit, fold, inflation and table rebuild (the plain scan:
carve, mark, inflation, table); beside them direct_cluster_last_ms; median of 20 calls after 3 warm-up calls.  Three situations:
  static   the same scan again (CONTINUE) on evidence that has saturated: nothing changes, no group of the grids is stored
  changed  map and evidence emptied (not timed), then the scan: every return is new, the table is rebuilt
  reset    the same scan with RESET: the evidence is cleared and written again, the map stays
The device's grids and stats are checked against the g++ -O2 build of the same headers on one host thread
(tests/evidence_harness.py) on a 4096-point subset (equality) on the way, and that program's time is recorded.
usage: evidence_bench.py [out.json]   (default profiles/evidence_bench.json)"""
import json
import os
import sys
import tempfile

import numpy as np
import torch  # before the library is loaded: torch must initialise its HIP runtime first

sys.path.insert(0, ".")
os.environ["DIRECT_CLUSTER_SCAN_TIMING"] = "1"
from direct_amd import cluster, problems  # noqa: E402
from tests import evidence_harness as eh  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "evidence_bench.json")
CALLS, WARM = 20, 3
RES, RANGE = 0.15, 10.0
MAPS = (((333, 333, 33), np.array([-25.0, -25.0, 0.0]), np.array([0.07, -0.04, 2.45])),
        ((1024, 1024, 16), np.array([-76.8, -76.8, 0.0]), np.array([0.07, -0.04, 1.25])))
SMALL = dict(max_batch=1, cluster_capacity=64, candidate_capacity=64)
PAR = eh.DEFAULTS
PLAIN_PHASES, EVID_PHASES = ("carve", "mark", "inflate", "table"), ("touch", "hit", "fold", "inflate", "table")

harness = eh.build(tempfile.mkdtemp())


def timed(gen, fn, phases, names, before=None):
    ev, phase = [], []
    for _ in range(WARM + CALLS):
        if before is not None:
            before()
        torch.cuda.synchronize()
        fn()
        ev.append(gen.last_ms())
        phase.append(phases())
    med = lambda v: round(float(np.median(v[WARM:])), 4)
    ph = np.array(phase[WARM:])
    out = dict(event_ms=med(ev), event_ms_min=round(float(min(ev[WARM:])), 4))
    out.update({name + "_ms": med(list(ph[:, k])) for k, name in enumerate(names)})
    return out


rows, ok = [], True
for dims, lower, origin in MAPS:
    upper = lower + np.array(dims) * RES
    empty = np.zeros(dims, np.uint8)
    plain, evid = cluster.ClusterGenerator(dims, **SMALL), cluster.ClusterGenerator(dims, **SMALL)
    for n in (100000, 1000000):
        pts = problems.make_point_cloud(dims, RES, lower, seed=11, n_points=n)
        dev_pts = torch.from_numpy(pts).to("cuda:0")
        for inflate in ((0, 0, 0), (2, 2, 1)):
            kw = dict(inflate=inflate, map_upper=upper, track_known=True)
            want = eh.run(harness, pts[:4096], origin, RANGE, PAR, inflate, "reset", track=True, dims=dims, res=RES, lower=lower, upper=upper)
            evid.set_map(empty)
            st = evid.integrate_scan_evidence(pts[:4096], origin, lower, RES, RANGE, mode="reset", **PAR, **kw)
            equal = bool(np.array_equal(evid.evidence_grid(), want["ev"]) and np.array_equal(evid.scan_grid(), want["raw"]) and
                         np.array_equal(evid.get_map(), want["map"]) and np.array_equal(evid.known_grid(), want["known"]) and
                         [st[k] for k in eh.STATS] == want["stats"].tolist())
            ok = ok and equal
            row = dict(map=list(dims), points=n, inflate=list(inflate), equal_to_host_program_on_4096_points=equal,
                       host_one_thread_ms_4096_points=round(want["ms"], 3))

            def p_scan(mode):
                return lambda: plain.integrate_scan(dev_pts, origin, lower, RES, RANGE, mode=mode, **kw)

            def e_scan(mode):
                return lambda: evid.integrate_scan_evidence(dev_pts, origin, lower, RES, RANGE, mode=mode, **PAR, **kw)

            def e_empty():
                evid.set_map(empty)
                evid.set_evidence(None)

            for situation in ("static", "changed", "reset"):
                cell = {}
                for run in (1, 2):   # plain, evidence, plain, evidence
                    if situation == "static":
                        p_scan("reset")()
                        cell["plain_%d" % run] = timed(plain, p_scan("continue"), plain.scan_phase_ms, PLAIN_PHASES)
                        e_scan("reset")()
                        for _ in range(6):   # 70 / 17 and 40 / 8: saturated on both sides after five scans
                            last = e_scan("continue")()
                        assert last["set"] + last["cleared"] == 0
                        cell["evidence_%d" % run] = timed(evid, e_scan("continue"), evid.evidence_phase_ms, EVID_PHASES)
                    elif situation == "changed":
                        cell["plain_%d" % run] = timed(plain, p_scan("reset"), plain.scan_phase_ms, PLAIN_PHASES, before=lambda: plain.set_map(empty))
                        cell["evidence_%d" % run] = timed(evid, e_scan("continue"), evid.evidence_phase_ms, EVID_PHASES, before=e_empty)
                    else:
                        cell["plain_%d" % run] = timed(plain, p_scan("reset"), plain.scan_phase_ms, PLAIN_PHASES)
                        cell["evidence_%d" % run] = timed(evid, e_scan("reset"), evid.evidence_phase_ms, EVID_PHASES)
                row[situation] = cell
                p, e = cell["plain_1"], cell["evidence_1"]
                print("%s %7d points, inflate %s, %-7s: plain %.3f / %.3f ms (carve %.3f, mark %.3f, inflate %.3f, table %.3f); evidence %.3f / %.3f ms "
                      "(touch %.3f, hit %.3f, fold %.3f, inflate %.3f, table %.3f)"
                      % (dims, n, inflate, situation, p["event_ms"], cell["plain_2"]["event_ms"], p["carve_ms"], p["mark_ms"], p["inflate_ms"],
                         p["table_ms"], e["event_ms"], cell["evidence_2"]["event_ms"], e["touch_ms"], e["hit_ms"], e["fold_ms"], e["inflate_ms"],
                         e["table_ms"]), flush=True)
            rows.append(row)
    plain.close()
    evid.close()

res = dict(resolution=RES, max_range=RANGE, params=PAR, calls=CALLS, warmup=WARM, device=torch.cuda.get_device_name(0),
           equal_to_host_program=ok, rows=rows)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"evidence_bench": res}, f, indent=1)
    f.write("\n")
print(json.dumps({"evidence_bench": {"rows": len(rows), "equal_to_host_program": ok}}))
sys.exit(0 if ok else 1)
