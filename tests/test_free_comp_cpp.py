"""direct_amd/csrc/free_comp_math.h as plain C++ (g++, tests/free_comp_harness.py): the result does not depend on the order of
the unions, the staleness key, the normal form of the floor, the forward offsets, and the shape of the sources.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import free_comp_harness as fh

CSRC = os.path.join(fh.ROOT, "direct_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return fh.build(tmp_path_factory.mktemp("free_comp_cpp"))


@pytest.mark.parametrize("name,grid", [("serpentine", fh.serpentine()), ("far_end", fh.far_end()), ("random", fh.random_map(fh.DIMS_BIG, 2)),
                                       ("chain", np.zeros((1024, 2, 2), np.uint8))], ids=["serpentine", "far_end", "random", "chain"])
def test_order_independence(exe, name, grid):
    """4.  the merge pass with its unions in lane order, reversed and in three shuffled orders: identical labels, sizes and stats"""
    first = fh.run(exe, grid)
    assert first["unions"] > 0
    for order in (1, 2, 3, 4):
        other = fh.run(exe, grid, order=order)
        fh.assert_same(other, first["label"], first["size"], first["stats"], what=(name, order))


def test_staleness_key_and_normal_floor(exe):
    """a set built without a floor outlives a field build but not a map change; one built with a floor outlives neither; no set
    serves nothing; min_d2 0 and 1 are one floor"""
    key = fh.run(exe, np.zeros((2, 2, 2), np.uint8))["key"]
    assert key.tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 0, 2]


def test_min_d2_one_is_the_plain_graph(exe):
    """min_d2 <= 1 reads no field: a field of zeros, which would close every voxel under any floor, changes nothing"""
    grid = fh.random_map(fh.DIMS, 2)
    plain = fh.run(exe, grid)
    fh.assert_same(fh.run(exe, grid, np.zeros(grid.shape, np.int32), 1), plain["label"], plain["size"], plain["stats"])
    assert fh.run(exe, grid, np.zeros(grid.shape, np.int32), 2)["stats"].tolist() == [0, 0, 0, -1]


def test_forward_offsets_are_the_positive_half():
    """the 13 forward offsets of the header: lexicographically positive, ascending, and with their negatives all 26"""
    offs = []
    for k in range(13):
        q = k + 14
        offs.append((q // 9 - 1, (q // 3) % 3 - 1, q % 3 - 1))
    assert offs == sorted(offs) and all(o > (0, 0, 0) for o in offs) and offs[0] == (0, 0, 1) and offs[-1] == (1, 1, 1)
    assert sorted(offs + [tuple(-v for v in o) for o in offs]) == sorted(fh.OFFSETS)
    txt = open(os.path.join(CSRC, "free_comp_math.h")).read()
    assert "const int q = k + 14;" in txt and "kForward = 13" in txt


def test_sources_keep_their_constraints():
    """integers only, every access to `parent` in k_cc_merge is an agent-scope atomic, and every loop of the union-find is bounded"""
    math = open(os.path.join(CSRC, "free_comp_math.h")).read()
    kern = open(os.path.join(CSRC, "free_comp.h")).read()
    code = re.sub(r"//[^\n]*", "", math + kern)
    assert not re.search(r"\b(float|double)\b", code)
    assert "while" not in code
    merge = re.sub(r"//[^\n]*", "", kern[kern.index("void k_cc_merge"):kern.index("void k_cc_flatten")])
    assert merge.count("__HIP_MEMORY_SCOPE_AGENT") == 2 and merge.count("A.label[") == 2   # the load and the min, nothing else
