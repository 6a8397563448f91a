"""Time of direct_cluster_cube_corridor_clear_batch for the 64 queries of tools/grid_path_bench.py on the 200 x 200 x 40 map, in
one process, timed by direct_cluster_last_ms (HIP events), median of 20 calls after 3 warm-up calls each, all on the
device-resident paths of ONE grid_paths_clear call with the floor:
  (a) the plain call, as the yardstick;
  (b) the clear call warm: its floor table resident;
  (c) the clear call cold: three floors alternating on two slots, so every call builds its table;
  (d) the table build alone: a cold call for ONE row of ONE voxel, against the table part of a change of map in the same run
      (direct_cluster_map_from_cloud adding no points: its timed part is then the counters' reset and the table build);
  (e) polytopes per row, plain against clear.
(b) must equal the g++ build of its arithmetic (tests/cube_corridor_harness.py, floor-filled) and, for the witness, the plain call of a
second handle holding the thresholded field as its map.
usage: cube_corridor_clear_bench.py [out.json]   (default profiles/cube_corridor_clear_bench.json)"""
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402,F401  (before the library is loaded)
from direct_amd import abi, cluster  # noqa: E402
from tests import cube_corridor_clear_harness as cl  # noqa: E402
from tests import grid_path_harness as gh  # noqa: E402
from tests.real_corridor_lib import LOWER, RES  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "cube_corridor_clear_bench.json")
CALLS, WARM, NQ, CAP, SEG = 20, 3, 64, 4096, 256
FLOOR, OTHERS = 4, (9, 16)

grid = gh.big_map()
starts, goals = gh.big_queries(grid, NQ)
gen = cluster.ClusterGenerator(grid.shape, max_batch=NQ, cluster_capacity=64, candidate_capacity=64)
gen.set_map(grid)
gen.build_distance_field()
d2 = gen.distance_field()
dev = gen.grid_paths_clear(starts, goals, FLOOR, path_capacity=CAP, mem="device")
rtn = dev["rtn"].cpu().numpy()
path_len = dev["path_len"].cpu().numpy()
pxyz, plen = dev["path_xyz"], dev["path_len"]


def timed(fn):
    ms, r = [], None
    for _ in range(WARM + CALLS):
        r = fn()
        ms.append(gen.last_ms())
    v = ms[WARM:]
    return r, dict(ms_median=round(float(np.median(v)), 4), ms_min=round(float(min(v)), 4), ms_max=round(float(max(v)), 4))


host = lambda r: {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in r.items()}
plain, row_a = timed(lambda: gen.cube_corridors(pxyz, plen, LOWER, RES, seg_capacity=SEG))
warm, row_b = timed(lambda: gen.cube_corridors_clear(pxyz, plen, LOWER, RES, FLOOR, seg_capacity=SEG))
assert warm["info"][0] == 0
cycle = [FLOOR] + list(OTHERS)
state = dict(i=1, built=0)   # the warm calls left FLOOR resident: start behind it, and every call of the cycle misses


def cold_call():
    r = gen.cube_corridors_clear(pxyz, plen, LOWER, RES, cycle[state["i"] % 3], seg_capacity=SEG)
    state["i"] += 1
    state["built"] += int(r["info"][0])
    return r


_, row_c = timed(cold_call)
assert state["built"] == WARM + CALLS
one_xyz, one_len = np.zeros((1, 1, 3), np.int32), np.ones(1, np.int32)
one_xyz[0, 0] = starts[0]
state.update(built=0)   # the cycle goes on


def build_alone():
    r = gen.cube_corridors_clear(one_xyz, one_len, LOWER, RES, cycle[state["i"] % 3], seg_capacity=1)
    state["i"] += 1
    state["built"] += int(r["info"][0])
    return r


_, row_d = timed(build_alone)
assert state["built"] == WARM + CALLS
_, row_d1 = timed(lambda: gen.cube_corridors_clear(one_xyz, one_len, LOWER, RES, cycle[(state["i"] - 1) % 3], seg_capacity=1))
_, row_m = timed(lambda: gen.set_map_from_cloud(np.zeros((0, 3), np.float32), LOWER, RES, cloud_margin=0.0, add=True))
assert np.array_equal(gen.get_map(), grid)
gen.close()

plain, warm = host(plain), host(warm)
want = cl.corridors(cl.build(tempfile.mkdtemp()), grid, d2, FLOOR, pxyz.cpu().numpy(), path_len, res=RES, lower=LOWER, seg_capacity=SEG)
for k in abi.CUBE_CORRIDOR_OUTPUTS:
    assert warm[k].tobytes() == want[k].tobytes(), k
other = cluster.ClusterGenerator(grid.shape, max_batch=1, cluster_capacity=64, candidate_capacity=64)
other.set_map((d2 < FLOOR).astype(np.uint8))
witness = other.cube_corridors(pxyz.cpu().numpy(), path_len, LOWER, RES, seg_capacity=SEG)
other.close()
for k in abi.CUBE_CORRIDOR_OUTPUTS:
    assert warm[k].tobytes() == witness[k].tobytes(), k

ok = rtn == cluster.GRID_PATH_OK
res = dict(queries=NQ, map=list(grid.shape), calls=CALLS, min_d2=FLOOR, cold_floors=cycle, paths_found=int(ok.sum()),
           path_voxels_total=int(path_len[ok].sum()), below_floor_voxels=int(warm["info"][1]), occupied_voxels=int((grid == 1).sum()),
           plain=row_a, clear_warm=row_b, clear_cold=row_c, table_build_one_voxel_row_cold=row_d, one_voxel_row_warm=row_d1,
           map_table_build=row_m,
           warm_inside_plain_spread=bool(row_a["ms_min"] <= row_b["ms_median"] <= row_a["ms_max"]),
           polytopes_plain=int(plain["n_seg"].sum()), polytopes_clear=int(warm["n_seg"].sum()),
           polytopes_per_row_plain=dict(mean=round(float(plain["n_seg"][ok].mean()), 2), max=int(plain["n_seg"].max())),
           polytopes_per_row_clear=dict(mean=round(float(warm["n_seg"][ok].mean()), 2), max=int(warm["n_seg"].max())),
           rows_overflowing=dict(plain=int((plain["rtn"] == cluster.CUBE_CORRIDOR_OVERFLOW).sum()),
                                 clear=int((warm["rtn"] == cluster.CUBE_CORRIDOR_OVERFLOW).sum())))
f = lambda r: "%.3f ms (min %.3f, max %.3f)" % (r["ms_median"], r["ms_min"], r["ms_max"])
print("64 queries, floor %d: plain %s; clear warm %s; clear cold %s; table build with a one-voxel row %s (the same row warm %s) against the "
      "map's table %s; polytopes plain %d, clear %d" % (FLOOR, f(row_a), f(row_b), f(row_c), f(row_d), f(row_d1), f(row_m),
                                                        res["polytopes_plain"], res["polytopes_clear"]), flush=True)
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as fo:
    json.dump({"cube_corridor_clear_bench": res}, fo, indent=1)
    fo.write("\n")
print(json.dumps({"cube_corridor_clear_bench": res}))
