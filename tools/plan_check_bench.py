"""Time of direct_cluster_plan_check_batch (k_plan_starts + k_plan_seg + k_plan_deep + k_plan_rows) on device-resident plans, from
direct_cluster_last_ms (HIP events): the median of 20 calls after 3 warm-up calls.
usage: plan_check_bench.py [out.json] [B] [N]   ->  one line per case; the JSON (key "plan_check_bench") goes to out.json
       (default profiles/plan_check_bench.json)
Plans: B = 4096 x N = 100 config-3 corridors solved on the device (20 fixed phase-1 iterations), float storage - the plans of
       tools/audit_bench.py case (a).  They run for 150 - 350 m, so the map is 1024 x 1024 x 16 voxels of 0.7 m around them.
Cases: "empty"   an empty map: the floor, every segment resolved by its root box;
       "D6/8/10" a cluttered synthetic map (problems.make_voxel_map: pillars, boxes, rings) at depth 6, 8 and 10.
       The plans were not solved in that map: the share of blocked rows is a property of the case, recorded with it.
For each case: blocked rows, the share of them with no depth-(D+3) dyadic point in an occupied voxel (the conservative ones, on a
sample), box tests per segment, the length of the unresolved list, and equality with the CPU harness's descent on a 64-row sample.
Yardsticks of the same run: direct_traj_audit_batch with every output on the same plans, and the harness's descent of all rows on
one host thread."""
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (before the library: torch initialises its HIP runtime first)

from direct_amd import abi, cluster, problems, solver  # noqa: E402
from tests import plan_check_harness as ph  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "plan_check_bench.json")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
N = int(sys.argv[3]) if len(sys.argv) > 3 else 100
CALLS, WARM = 23, 3
DIMS, RES = (1024, 1024, 16), 0.7
LOWER = np.array([-0.5 * DIMS[0] * RES, -0.5 * DIMS[1] * RES, -4.0])
SAMPLE, CONS_SAMPLE = 64, 24
dev = torch.device("cuda", 0)

batch = problems.make_batch("corridor", B, N, seed=1000)
s = solver.DdpSolver(B, N, batch.p_max, np.float64)
_, plan = s.plan(abi.phase0_params(), abi.phase1_params(iter_max=20, fixed_iters=1), batch)
s.close()
host = dict(n_seg=np.ascontiguousarray(batch.n_seg, np.int32), T=np.ascontiguousarray(plan.T, np.float32),
            poly=np.ascontiguousarray(plan.poly, np.float32))
up = lambda a: torch.from_numpy(a).to(dev)
dv = {k: up(v) for k, v in host.items()}


def audit_ms():
    """direct_traj_audit_batch with every output on the same plans (tools/audit_bench.py case a)"""
    keep = dict(dv, cost=up(np.ascontiguousarray(plan.cost, np.float32)), rtn=up(np.ascontiguousarray(plan.rtn, np.int32)),
                n_planes=up(np.ascontiguousarray(batch.n_planes, np.int32)), planes=up(np.ascontiguousarray(batch.planes, np.float32)))
    cin, cout = abi.AuditIn(), abi.AuditOut()
    cin.batch, cin.n_seg_max, cin.mem, cin.p_max = B, N, abi.MEM_DEVICE, batch.p_max
    cin.max_vel, cin.max_acc, cin.max_jerk, cin.clearance = 2.0, 2.0, 10.0, 0.0
    for k, v in keep.items():
        setattr(cin, k, v.data_ptr())
    shapes = dict(c_where=(B, 2), at=(B, 4), seg_peak=(B, N, 4), gap=(B, 3), best=(1,))
    ints = ("c_where", "verdict", "best")
    o = {"status": torch.zeros(B, dtype=torch.int32, device=dev)}
    for k in abi.AUDIT_OUTPUTS:
        o[k] = torch.zeros(shapes.get(k, (B,)), dtype=(torch.int64 if k == "best" else torch.int32) if k in ints else torch.float32, device=dev)
    for k, v in o.items():
        setattr(cout, k, v.data_ptr())
    h = solver.DdpSolver(1, N, batch.p_max, np.float32)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    ms = []
    for _ in range(CALLS):
        h.audit_device(cin, cout)
        ms.append(h.audit_last_ms())
    torch.cuda.synchronize()
    h.close()
    return float(np.median(ms[WARM:]))


def dense_hit(rows, depth, grid):
    """for each row: does a dyadic point of `depth` of any segment lie in an occupied voxel?"""
    out = []
    for b in rows:
        n = int(host["n_seg"][b])
        P = np.stack([ph.control_points(host["poly"][b, i], host["T"][b, i], True) for i in range(n)])
        for _ in range(depth):
            P = ph.halve_all(P)
        pts = np.concatenate([P[:, :, 0], P[:, :, 5]])
        out.append(bool(ph.voxel_bytes(pts, grid, LOWER, RES).any()))
    return np.array(out, bool)


def run(name, gen, grid, depth, harness):
    kw = dict(map_lower=LOWER, resolution=RES, depth=depth)
    ms = []
    for _ in range(CALLS):
        out = gen.check_plans(dv["n_seg"], dv["T"], poly=dv["poly"], **kw)
        ms.append(gen.last_ms())
    med = float(np.median(ms[WARM:]))
    cnt = gen.check_plans(dv["n_seg"], dv["T"], poly=dv["poly"], count=True, **kw)
    got = {k: out[k].cpu().numpy() for k in ph.KEYS}
    sample = np.linspace(0, B - 1, min(SAMPLE, B)).astype(int)
    want, _ = ph.run(harness, {k: v[sample] for k, v in host.items()}, grid, depth, lower=LOWER, res=RES)
    ph.assert_same({k: v[sample] for k, v in got.items()}, want, name)          # equality with the harness
    _, info = ph.run(harness, host, grid, depth, lower=LOWER, res=RES, reps=3)
    blocked = np.flatnonzero(got["verdict"] > 0)
    cons = blocked[:: max(1, len(blocked) // CONS_SAMPLE)][:CONS_SAMPLE]
    hit = dense_hit(cons, depth + 3, grid) if len(cons) else np.zeros(0, bool)
    segs = int(host["n_seg"].sum())
    res = dict(case=name, rows=B, segments=N, depth=depth, occupied_voxels=int(grid.sum()), ms=round(med, 4), ms_min=round(float(min(ms[WARM:])), 4),
               ms_max=round(float(max(ms[WARM:])), 4), valid_rows=int((got["status"] == 0).sum()), blocked_rows=int(len(blocked)),
               blocked_share=round(len(blocked) / B, 4), conservative_sampled=int(len(cons)), conservative=int((~hit).sum()),
               box_tests_per_segment=round(cnt["box_tests"] / segs, 3), unresolved_list=cnt["unresolved"],
               harness_equal_rows=int(len(sample)), harness_one_thread_ms=round(info["ms"], 3),
               harness_box_tests_per_segment=round(info["tests"] / segs, 3))
    print("%-5s B=%d N=%d D=%d: %.3f ms (min %.3f, max %.3f); blocked %d rows, conservative %d of %d sampled; %.2f box tests per segment, "
          "%d slots unresolved; one host thread %.1f ms" % (name, B, N, depth, med, res["ms_min"], res["ms_max"], len(blocked), res["conservative"],
                                                          len(cons), res["box_tests_per_segment"], cnt["unresolved"], info["ms"]), flush=True)
    return res


harness = ph.build(tempfile.mkdtemp(prefix="plan_check_bench_"))
gen = cluster.ClusterGenerator(DIMS, max_batch=1, cluster_capacity=64, candidate_capacity=64)
empty = np.zeros(DIMS, np.uint8)
gen.set_map(empty)
results = [run("empty", gen, empty, 8, harness)]
clutter, _ = problems.make_voxel_map(DIMS, seed=7, n_pillars=1000, n_boxes=400, n_rings=100)
gen.set_map(clutter)
for D in (6, 8, 10):
    results.append(run("D%d" % D, gen, clutter, D, harness))
gen.close()
a_ms = audit_ms()
d8 = next(r for r in results if r["case"] == "D8")
summary = dict(audit_every_output_ms=round(a_ms, 4), check_D8_ms=d8["ms"], check_over_audit=round(d8["ms"] / a_ms, 3),
               goal_met=bool(d8["ms"] <= a_ms))
print("audit with every output on the same plans: %.3f ms; the check at D = 8: %.3f ms (%.2f x)" % (a_ms, d8["ms"], d8["ms"] / a_ms), flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"plan_check_bench": dict(cases=results, yardstick=summary)}, f, indent=1)
    f.write("\n")
print(json.dumps({"plan_check_bench": dict(cases=results, yardstick=summary)}))
