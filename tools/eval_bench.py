"""Throughput of direct_traj_eval_batch (k_eval_starts + k_eval) on device-resident arrays, timed by
direct_traj_eval_last_ms.  Plans: free-space corridors solved on the device (20 fixed phase-1 iterations), tiled to B rows.
usage: eval_bench.py [B] [N] [M]   ->  one line per case, and a JSON summary line (key "eval_bench")
Cases: (1) B x M grid queries, every output but state (pos .. snap + seg), float storage - the headline; (2) the same
with explicit times (the grid's own values); (3) the headline in double storage; (4) one row of 2^20 grid queries; (5) a coarse
grid, M / 8 queries per row: every chunk spans more segments than k_eval stages in LDS (the per-query path).  "fallback" is
the share of chunks that take that path, from the plans' own segment start times."""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (before the library: torch initialises its HIP runtime first)

from direct_amd import abi, problems, solver  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100
M = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
dev = torch.device("cuda", 0)
OUTS = ("seg", "pos", "vel", "acc", "jerk", "snap")
nb = min(B, 4096)
batch = problems.make_batch("free", nb, N, seed=1000)
s = solver.DdpSolver(nb, N, batch.p_max, np.float64)
_, plan = s.plan(abi.phase0_params(), abi.phase1_params(iter_max=20, fixed_iters=1), batch)
s.close()
ok = plan.rtn >= 0
CHUNK, SLOTS = 256, 32   # kEvalChunk, kEvalSlots of direct_amd/csrc/traj_eval.h


def fallback_share(rows, m, dt):
    """share of the chunks of a grid t_j = j dt whose queries span more than SLOTS segments (rows tile the nb plans)"""
    n_fb = n_all = 0
    for b in range(min(rows, nb)):
        n = int(batch.n_seg[b])
        S = np.concatenate([[0.0], np.cumsum(plan.T[b, :n].astype(np.float64))])
        seg = np.searchsorted(S[:n], np.minimum(np.arange(m) * dt, S[n]), side="right") - 1
        seg = np.pad(seg, (0, -m % CHUNK), mode="edge").reshape(-1, CHUNK)
        n_fb += int((seg.max(1) - seg.min(1) + 1 > SLOTS).sum())
        n_all += seg.shape[0]
    return n_fb / n_all


def run(name, dtype, rows, m, explicit):
    td = torch.float64 if dtype == np.float64 else torch.float32
    rep = -(-rows // nb)
    n_seg = torch.from_numpy(np.tile(batch.n_seg, rep)[:rows]).to(dev)
    T = torch.from_numpy(np.tile(plan.T, (rep, 1))[:rows].astype(dtype)).to(dev)
    bez = torch.from_numpy(np.tile(plan.bez, (rep, 1, 1))[:rows].astype(dtype)).to(dev)
    Tsum = float(plan.T[ok].sum(1).min())
    dt = Tsum / m   # every query inside the trajectory
    cin, cout = abi.EvalIn(), abi.EvalOut()
    cin.batch, cin.n_seg_max, cin.m_max, cin.mem = rows, N, m, abi.MEM_DEVICE
    cin.n_seg, cin.T, cin.bez, cin.t0, cin.dt = n_seg.data_ptr(), T.data_ptr(), bez.data_ptr(), 0.0, dt
    t = None
    if explicit:
        t = (torch.arange(m, dtype=torch.float64, device=dev) * dt).to(td).expand(rows, m).contiguous()
        cin.t = t.data_ptr()
    o = {"status": torch.zeros(rows, dtype=torch.int32, device=dev)}
    for k in OUTS:
        o[k] = torch.empty((rows, m), dtype=torch.int32, device=dev) if k == "seg" else torch.empty((rows, m, 3), dtype=td, device=dev)
    for k, v in o.items():
        setattr(cout, k, v.data_ptr())
    s = solver.DdpSolver(1, N, batch.p_max, dtype)
    s.set_stream(torch.cuda.current_stream().cuda_stream)
    ms = []
    for _ in range(12):
        s.evaluate_device(cin, cout)
        ms.append(s.eval_last_ms())
    s.close()
    isz = np.dtype(dtype).itemsize
    written = rows * m * (4 + 5 * 3 * isz) + rows * 4
    read = rows * N * 19 * isz + rows * 4 + (rows * m * isz if explicit else 0)
    med = float(np.median(ms[2:]))
    assert (o["status"] == 0).all().item() or not ok.all()
    res = dict(case=name, rows=rows, queries=m, dtype=np.dtype(dtype).name, explicit=bool(explicit),
               fallback=round(fallback_share(rows, m, dt), 4), ms=round(med, 4),
               ms_min=round(float(min(ms[2:])), 4), ms_max=round(float(max(ms[2:])), 4), written_gb=round(written / 1e9, 4),
               read_gb=round(read / 1e9, 4), write_tb_s=round(written / med / 1e9, 3), gqueries_s=round(rows * m / med / 1e6, 2))
    print("%-9s B=%d m=%d %s%s: %.3f ms (min %.3f, max %.3f) -> %.2f TB/s written (%.2f GB), %.1f G queries/s, fallback %.3f"
          % (name, rows, m, res["dtype"], " explicit" if explicit else " grid", med, res["ms_min"], res["ms_max"],
             res["write_tb_s"], written / 1e9, res["gqueries_s"], res["fallback"]), flush=True)
    del o, t
    torch.cuda.empty_cache()
    return res


results = [run("headline", np.float32, B, M, False), run("explicit", np.float32, B, M, True),
           run("f64", np.float64, B, M, False), run("one_row", np.float32, 1, 1 << 20, False),
           run("coarse", np.float32, B, max(M // 8, 1), False)]
print(json.dumps({"eval_bench": results}))
