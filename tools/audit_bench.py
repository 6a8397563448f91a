"""Time of direct_traj_audit_batch (k_audit_starts + k_audit_items + k_audit_rows + k_audit_best) on device-resident arrays,
timed by direct_traj_audit_last_ms (HIP events), and next to it the time of direct_traj_sample_batch with cmax at dt = 0.1 on
the same inputs - what callers use today; it computes something else (maxima over samples), so it is context, not a ratio.
usage: audit_bench.py [out.json] [Ba] [Bb] [N]   ->  one line per case; the JSON (key "audit_bench") goes to out.json
       (default profiles/audit_bench.json)
Cases: (a) Ba = 4096 plans x N = 100 segments in corridors of 6-12 planes, float storage, every output;
       (b) Bb = 32768 x 100, no corridor, the per-axis outputs only (no norm items).
Plans: config-3 corridors solved on the device (20 fixed phase-1 iterations), tiled to the rows of a case.
"flops" are COUNTED from the ladder's trip counts (traj_audit_math.h), not measured: an fma is 2."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (before the library: torch initialises its HIP runtime first)

from direct_amd import abi, problems, solver  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "audit_bench.json")
BA = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
BB = int(sys.argv[3]) if len(sys.argv) > 3 else 32768
N = int(sys.argv[4]) if len(sys.argv) > 4 else 100
CALLS, WARM = 24, 4
FP64_VECTOR_PEAK = 78.6e12   # MI355X data sheet: FP64 vector
HALVINGS = 30                # audit::kHalvings
dev = torch.device("cuda", 0)
nb = min(BA, 4096)
batch = problems.make_batch("corridor", nb, N, seed=1000)
s = solver.DdpSolver(nb, N, batch.p_max, np.float64)
_, plan = s.plan(abi.phase0_params(), abi.phase1_params(iter_max=20, fixed_iters=1), batch)
s.close()


def ladder_flops(M):
    """levels m = 1..M: m pieces, each (HALVINGS + 1) Horner evaluations of degree m and HALVINGS midpoints (add, multiply)"""
    return sum(m * ((HALVINGS + 1) * 2 * m + HALVINGS * 2) + (m + 1) for m in range(1, M + 1))


def item_flops(norms, planes_per_segment):
    axis = sum(3 * (ladder_flops(4 - k) + (6 - k) * (2 * (5 - k) + 3)) for k in (1, 2, 3))
    norm = sum(ladder_flops(2 * (5 - k) - 1) + (2 * (5 - k) + 1) * (6 * (5 - k) + 7) + 6 * (5 - k) ** 2 for k in (1, 2, 3)) if norms else 0
    plane = ladder_flops(4) + 6 * 13 + 6 * 5
    return axis + norm + planes_per_segment * plane


def run(name, dtype, rows, corridor, outputs):
    td = torch.float64 if dtype == np.float64 else torch.float32
    rep = -(-rows // nb)
    tile = lambda a: np.tile(a, (rep,) + (1,) * (a.ndim - 1))[:rows]
    up = lambda a, dt_: torch.from_numpy(np.ascontiguousarray(tile(a), dt_)).to(dev)
    keep = dict(n_seg=up(batch.n_seg, np.int32), T=up(plan.T, dtype), poly=up(plan.poly, dtype), cost=up(plan.cost, dtype),
                rtn=up(plan.rtn, np.int32))
    cin, cout = abi.AuditIn(), abi.AuditOut()
    cin.batch, cin.n_seg_max, cin.mem = rows, N, abi.MEM_DEVICE
    cin.max_vel, cin.max_acc, cin.max_jerk, cin.clearance = 2.0, 2.0, 10.0, 0.0
    if corridor:
        keep["n_planes"], keep["planes"] = up(batch.n_planes, np.int32), up(batch.planes, dtype)
        cin.p_max = batch.p_max
    for k, v in keep.items():
        setattr(cin, k, v.data_ptr())
    shapes = dict(c_where=(rows, 2), at=(rows, 4), seg_peak=(rows, N, 4), gap=(rows, 3), best=(1,))
    ints = ("c_where", "verdict", "best")
    o = {"status": torch.zeros(rows, dtype=torch.int32, device=dev)}
    for k in outputs:
        o[k] = torch.zeros(shapes.get(k, (rows,)), dtype=(torch.int64 if k == "best" else torch.int32) if k in ints else td, device=dev)
    for k, v in o.items():
        setattr(cout, k, v.data_ptr())
    h = solver.DdpSolver(1, N, batch.p_max, dtype)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    ms = []
    for _ in range(CALLS):
        h.audit_device(cin, cout)
        ms.append(h.audit_last_ms())
    med = float(np.median(ms[WARM:]))
    # the context figure: the sampler's maxima over samples on the same plans (it reads control points)
    bez = up(plan.bez, dtype)
    cap = int(plan.T.sum(1).max() / 0.1) + 2 * N + 8
    si, so = abi.SampleIn(), abi.SampleOut()
    si.batch, si.n_seg_max, si.capacity, si.derivs, si.mem, si.dt = rows, N, cap, 2, abi.MEM_DEVICE, 0.1
    si.n_seg, si.bez, si.T = keep["n_seg"].data_ptr(), bez.data_ptr(), keep["T"].data_ptr()
    sk = dict(count=torch.zeros(rows, dtype=torch.int32, device=dev))
    for k in ("pos", "vel", "acc"):
        sk[k] = torch.empty((rows, cap, 3), dtype=td, device=dev)
    for k in ("vmax", "amax") + (("cmax",) if corridor else ()):
        sk[k] = torch.zeros(rows, dtype=td, device=dev)
    if corridor:
        si.p_max, si.n_planes, si.planes = batch.p_max, keep["n_planes"].data_ptr(), keep["planes"].data_ptr()
    for k, v in sk.items():
        setattr(so, k, v.data_ptr())
    sms = []
    for _ in range(8):
        h.sample_device(si, so)
        sms.append(h.sample_last_ms())
    torch.cuda.synchronize()
    st = o["status"].cpu().numpy()
    n_pl = int(tile(batch.n_planes).sum()) if corridor else 0
    segs = int(tile(batch.n_seg).sum())
    norms = any(k in outputs for k in ("vnorm", "anorm", "jnorm"))
    items = segs * (9 + (3 if norms else 0)) + n_pl
    flops = segs * item_flops(norms, 0) + n_pl * item_flops(False, 1) - n_pl * item_flops(False, 0)
    res = dict(case=name, rows=rows, segments=N, dtype=np.dtype(dtype).name, corridor=bool(corridor), outputs=list(outputs),
               valid_rows=int((st == 0).sum()), ms=round(med, 4), ms_min=round(float(min(ms[WARM:])), 4), ms_max=round(float(max(ms[WARM:])), 4),
               items=items, gitems_s=round(items / med / 1e6, 3), counted_gflop=round(flops / 1e9, 3),
               counted_tflops=round(flops / med / 1e9, 3), share_of_fp64_vector_peak=round(flops / med / 1e-3 / FP64_VECTOR_PEAK, 4),
               sampler_dt01_ms=round(float(np.median(sms[2:])), 4))
    if "verdict" in o:
        v = o["verdict"].cpu().numpy()
        res["rows_passing"] = int((v == 0).sum())
    print("%-3s B=%d N=%d %s%s: %.3f ms (min %.3f, max %.3f), %.2f G items/s, counted %.1f Tflop/s = %.1f %% of the fp64 vector peak; "
          "sampler at dt = 0.1: %.3f ms" % (name, rows, N, res["dtype"], " corridor" if corridor else "", med, res["ms_min"], res["ms_max"],
                                           res["gitems_s"], res["counted_tflops"], 100 * res["share_of_fp64_vector_peak"],
                                           res["sampler_dt01_ms"]), flush=True)
    h.close()
    del o, sk, keep, bez
    torch.cuda.empty_cache()
    return res


results = [run("a", np.float32, BA, True, abi.AUDIT_OUTPUTS),
           run("b", np.float32, BB, False, ("t_total", "vpeak", "apeak", "jpeak", "at", "seg_peak", "gap", "verdict", "slowdown"))]
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump({"audit_bench": results}, f, indent=1)
    f.write("\n")
print(json.dumps({"audit_bench": results}))
