"""The lock-step walk through the EXISTING calls - TEST INFRASTRUCTURE of tests/test_gpu_cluster_corridor.py and
tools/cluster_corridor_bench.py: polyhedronGenerator::walk restated after lock_step_walk of tests/test_gpu_cube_corridor.py, every
round one polygon_generation(seeds, itr_inflate_max, itr_cluster_max) for the seeds that are due (in chunks of the handle's
max_batch) and one hull_planes() on the resident clusters with plane_capacity = p_max.  The result comes in the arrays of
ClusterGenerator.cluster_corridors, so that the two can be compared byte for byte."""
import numpy as np

from direct_amd import cluster


def lock_step_walk(gen, paths, lower, res, pop_back, itr_cluster_max, itr_inflate_max=1000, seg_capacity=12, p_max=20, dtype=np.float64):
    """paths: list of [n][3] voxel arrays, all inside the map and not empty -> dict(n_seg, n_planes, planes, seeds, centers, rtn,
    stats: dict(rounds, due_seeds, pops, device_ms))"""
    lower = [float(v) for v in lower]

    def outside(cur, pl):
        return any(cur[0] * p[0] + cur[1] * p[1] + cur[2] * p[2] + p[3] > 0.01 for p in pl)

    B, S, P = len(paths), int(seg_capacity), int(p_max)
    cor = [[] for _ in paths]
    nxt, lst, code = [0] * B, [None] * B, [cluster.CLUSTER_CORRIDOR_OK] * B
    done = [False] * B
    rounds = due_total = pops = 0
    device_ms = 0.0   # direct_cluster_last_ms summed over the device calls
    while True:
        due = []
        for b, p in enumerate(paths):
            while not done[b] and nxt[b] < len(p):
                cur = [int(p[nxt[b]][a]) * res + 0.5 * res + lower[a] for a in range(3)]
                if cur == lst[b]:
                    nxt[b] += 1
                    continue
                if pop_back and len(cor[b]) > 1 and not outside(cur, cor[b][-2]["planes"]):
                    cor[b].pop()
                    pops += 1
                if not cor[b] or outside(cur, cor[b][-1]["planes"]):
                    if len(cor[b]) >= S:
                        code[b], done[b] = cluster.CLUSTER_CORRIDOR_OVERFLOW, True
                        break
                    due.append((b, cur))
                    break
                lst[b] = cur
                nxt[b] += 1
        if not due:
            break
        rounds += 1
        due_total += len(due)
        for lo in range(0, len(due), gen.max_batch):
            part = due[lo:lo + gen.max_batch]
            seeds = np.array([paths[b][nxt[b]] for b, _ in part], np.int32)
            g = gen.polygon_generation(seeds, itr_inflate_max=itr_inflate_max, itr_cluster_max=itr_cluster_max, fetch_clusters=False)
            device_ms += gen.last_ms()
            h = gen.hull_planes(res, lower, batch=len(part), plane_capacity=P, vertex_capacity=1, want=("planes", "center"))
            device_ms += gen.last_ms()
            for i, (b, cur) in enumerate(part):
                if g["rtn"][i] == cluster.CLUSTER_OK and h["rtn"][i] == cluster.HULL_OVERFLOW and h["n_planes"][i] > P:
                    code[b], done[b] = cluster.CLUSTER_CORRIDOR_TOO_MANY_PLANES, True
                elif g["rtn"][i] != cluster.CLUSTER_OK or h["rtn"][i] != cluster.HULL_OK:
                    code[b], done[b] = cluster.CLUSTER_CORRIDOR_NO_POLYTOPE, True
                else:
                    cor[b].append(dict(planes=h["planes"][i].tolist(), center=h["center"][i].copy(), seed=cur))
                    lst[b] = cur
                    nxt[b] += 1
    out = dict(n_seg=np.zeros(B, np.int32), n_planes=np.zeros((B, S), np.int32), planes=np.zeros((B, S, P, 4), np.float64),
               seeds=np.zeros((B, S, 3), np.float64), centers=np.zeros((B, S, 3), np.float64), rtn=np.array(code, np.int32))
    for b in range(B):
        out["n_seg"][b] = len(cor[b])
        for s, c in enumerate(cor[b]):
            out["n_planes"][b, s] = len(c["planes"])
            out["planes"][b, s, :len(c["planes"])] = c["planes"]
            out["seeds"][b, s], out["centers"][b, s] = c["seed"], c["center"]
    for k in ("planes", "seeds", "centers"):
        out[k] = out[k].astype(dtype)   # float: one rounding of the double
    out["stats"] = dict(rounds=rounds, due_seeds=due_total, pops=pops, device_ms=device_ms)
    return out
