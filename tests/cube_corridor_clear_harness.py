"""What belongs to direct_cluster_cube_corridor_clear_batch alone - TEST INFRASTRUCTURE of tests/test_cube_corridor_clear_cpp.py,
tests/test_gpu_cube_corridor_clear.py and tools/cube_corridor_clear_bench.py.  The call's serial restatement is the one program of
tests/cube_corridor_harness.py with its table filled through direct_amd/csrc/cube_corridor_clear_math.h: table() and corridors()
here ask for that.  A second, stand-alone program drives the slot choice of the cache (floor_slot_choose).  Beside them the
reference field, the thresholded map of the independent witness, and the integer guarantee."""
import subprocess

import numpy as np

from tests import cpp_program as cpp
from tests import cube_corridor_harness as ch

build = ch.build

# floor_slot_choose driven as a handle drives it: lines "min_d2 serial" on stdin -> "slot hit" per line
SLOTS = r'''
#include <cstdio>
#include "cube_corridor_clear_math.h"
namespace cc = direct::cubecor;
int main() {
  cc::FloorSlot s[cc::kFloorSlots] = {};
  unsigned long long clock = 0, serial;
  int min_d2;
  while (scanf("%d %llu", &min_d2, &serial) == 2) {
    int hit = -1;
    const int k = cc::floor_slot_choose(s, cc::kFloorSlots, min_d2, serial, &hit);
    if (k < 0 || k >= cc::kFloorSlots) return 1;
    if (!hit) { s[k].min_d2 = min_d2; s[k].serial = serial; s[k].valid = 1; }
    s[k].used = ++clock;
    printf("%d %d\n", k, hit);
  }
  return 0;
}
'''


def build_slots(workdir):
    return cpp.compile_program(workdir, "floor_slots", SLOTS, ["-Wno-unknown-pragmas"])


def slot_choices(exe, calls):
    """calls: [(min_d2, serial)] in order -> [(slot, hit)]"""
    out = subprocess.run([exe], input="".join("%d %d\n" % c for c in calls), capture_output=True, text=True, check=True).stdout.split()
    return [(int(out[i]), int(out[i + 1])) for i in range(0, len(out), 2)]


def brute_d2(grid):
    """the exact squared distance of every voxel to the nearest occupied one, by NumPy brute force (uncapped; the map is not empty)"""
    occ = np.argwhere(np.asarray(grid) == 1).astype(np.int64)
    idx = np.indices(grid.shape).reshape(3, -1).T.astype(np.int64)
    best = np.full(len(idx), np.iinfo(np.int64).max)
    for o in occ:
        best = np.minimum(best, ((idx - o) ** 2).sum(1))
    return best.reshape(grid.shape).astype(np.int32)


def thresholded(d2, min_d2):
    """the map on which the PLAIN call gives the clear call's result"""
    return (np.asarray(d2) < min_d2).astype(np.uint8)


def table(harness, grid, d2, min_d2):
    """-> the table in use [(X+1)][(Y+1)][(Z+1)]"""
    return ch.table(harness, grid, floor=(d2, min_d2))


def corridors(harness, grid, d2, min_d2, paths, path_len, res=ch.RES, lower=ch.LOWER, itr=1000, pop_back=True, seg_capacity=40, p_max=6,
              dtype=np.float64):
    """the outputs of ClusterGenerator.cube_corridors_clear for the same arguments (without info), plus queries"""
    return ch.corridors(harness, grid, paths, path_len, res, lower, itr, pop_back, seg_capacity, p_max, dtype, floor=(d2, min_d2))


def guarantee(cube_idx, n_seg, seeds_vox, d2, min_d2):
    """the integer guarantee: every voxel of every kept cube other than its seed voxel has d2 >= min_d2.  seeds_vox [B][S][3] are
    the seed voxels.  -> (cubes checked, cubes larger than one voxel)"""
    checked = large = 0
    for b in range(len(n_seg)):
        for k in range(min(int(n_seg[b]), cube_idx.shape[1])):
            c, s = cube_idx[b, k], seeds_vox[b, k]
            blk = d2[c[0]:c[3] + 1, c[1]:c[4] + 1, c[2]:c[5] + 1].copy()
            assert (c[:3] <= s).all() and (s <= c[3:]).all(), (b, k)
            blk[tuple(s - c[:3])] = np.iinfo(np.int32).max
            assert blk.min() >= min_d2, (b, k, c.tolist(), int(blk.min()))
            checked += 1
            large += blk.size > 1
    return checked, large
