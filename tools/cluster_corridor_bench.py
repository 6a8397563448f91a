"""Time of direct_cluster_corridor_batch against the lock-step walk through the existing calls (tests/cluster_corridor_lib.py:
polygon_generation + hull_planes per round, planes read back, the walk on the host) on the same handle and the same paths, in one
process.  Both sides are timed with a host clock around work that ends in a device synchronise (the lock-step walk is many calls,
so no event pair spans it); the new call's direct_cluster_last_ms and the lock-step walk's summed direct_cluster_last_ms are given
beside them.  Medians over RUNS runs after one warm-up run each; the outputs of the two must be identical bytes.
  (a) the 64 real paths of tests/real_corridor_lib.py on the 200 x 200 x 40 map;
  (b) 1024 goals from one start through grid_paths_fan (device-resident paths for the new call).
The lock-step walk here is the Python restatement: its host share is Python's, which the C++ mirror's would undercut; the
device_ms column does not depend on that.
usage: cluster_corridor_bench.py [out.json]   (default profiles/cluster_corridor_bench.json)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402,F401  (before the library is loaded)
from direct_amd import cluster, problems  # noqa: E402
from tests import cluster_corridor_lib as kl  # noqa: E402
from tests import real_corridor_lib as rl  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "cluster_corridor_bench.json")
RUNS_A, RUNS_B, SEG, PMAX, ITR = 5, 3, 64, 128, 50
RES, LOWER = rl.RES, rl.LOWER
KEYS = ("n_seg", "n_planes", "planes", "seeds", "centers", "rtn")


def real_paths(grid, n_paths=64):
    """the paths of real_corridor_batch, as voxel indices"""
    rng = np.random.default_rng(5)
    paths = []
    while len(paths) < n_paths:
        z = int(rng.integers(4, 30))
        free = np.argwhere(grid[:, :, z] == 0)
        a, b = free[rng.integers(len(free))], free[rng.integers(len(free))]
        if np.abs(a - b).sum() > 120:
            p = rl.grid_path(grid, [a[0], a[1], z], [b[0], b[1], z])
            if p is not None:
                paths.append(np.floor((p - LOWER) / RES).astype(np.int32))
    return paths


def pack(paths):
    cap = max(len(p) for p in paths)
    xyz, n = np.zeros((len(paths), cap, 3), np.int32), np.zeros(len(paths), np.int32)
    for b, p in enumerate(paths):
        xyz[b, :len(p)], n[b] = p, len(p)
    return xyz, n


def timed(fn, runs):
    wall, r = [], None
    for _ in range(1 + runs):
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    v = wall[1:]
    return r, dict(ms_median=round(float(np.median(v)), 3), ms_min=round(float(min(v)), 3), ms_max=round(float(max(v)), 3), runs=runs)


def compare(gen, name, paths, xyz_dev, n_dev, runs):
    xyz, n = pack(paths)
    last = []

    def new_call():
        r = gen.cluster_corridors(xyz_dev, n_dev, LOWER, RES, itr_cluster_max=ITR, seg_capacity=SEG, p_max=PMAX)
        last.append(gen.last_ms())
        return r

    got, t_new = timed(new_call, runs)
    want, t_old = timed(lambda: kl.lock_step_walk(gen, paths, LOWER, RES, True, ITR, seg_capacity=SEG, p_max=PMAX), runs)
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items() if k != "stats"}
    same = all(host[k].tobytes() == want[k].tobytes() for k in KEYS)
    row = dict(rows=len(paths), path_capacity=int(xyz.shape[1]), polytopes=int(host["n_seg"].sum()), polytopes_max=int(host["n_seg"].max()),
               planes_max=int(host["n_planes"].max()), codes=sorted(set(host["rtn"].tolist())), identical_bytes=bool(same), stats=got["stats"],
               new_call_wall=t_new, new_call_last_ms_median=round(float(np.median(last[1:])), 3), lock_step_wall=t_old,
               lock_step_device_ms=round(want["stats"]["device_ms"], 3), lock_step_rounds=want["stats"]["rounds"],
               lock_step_due=want["stats"]["due_seeds"])
    print(name, json.dumps(row), flush=True)
    assert same, name
    return row


grid, _ = problems.make_voxel_map((200, 200, 40), seed=7, n_pillars=170, n_boxes=70, n_rings=12)
gen = cluster.ClusterGenerator(grid.shape, max_batch=64, cluster_capacity=50000, candidate_capacity=10000)
gen.set_map(grid)
res = dict(map=list(grid.shape), itr_cluster_max=ITR, seg_capacity=SEG, p_max=PMAX, max_batch=64)

paths = real_paths(grid)
xyz, n = pack(paths)
res["real_64"] = compare(gen, "real_64", paths, torch.from_numpy(xyz).to("cuda:0"), torch.from_numpy(n).to("cuda:0"), RUNS_A)

z = 12
free = np.argwhere(grid[:, :, z] == 0)
rng = np.random.default_rng(11)
start = free[rng.integers(len(free))]
goals = np.array([[g[0], g[1], z] for g in free[rng.integers(len(free), size=1024)]], np.int32)
fan = gen.grid_paths_fan(np.array([[start[0], start[1], z]], np.int32), goals, path_capacity=512, mem="device")
ok = (fan["rtn"] == cluster.GRID_PATH_OK).cpu().numpy()
assert ok.all(), "a goal of the fan has no path"
fx, fn_ = fan["path_xyz"].cpu().numpy(), fan["path_len"].cpu().numpy()
fan_paths = [fx[b, :fn_[b]].copy() for b in range(len(fn_))]
res["fan_1024"] = compare(gen, "fan_1024", fan_paths, fan["path_xyz"], fan["path_len"], RUNS_B)
gen.close()
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print("written", OUT)
