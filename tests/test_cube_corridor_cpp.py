"""direct_amd/csrc/cube_corridor_math.h compiled by g++ -Wall -Werror (tests/cube_corridor_harness.py): the properties of the call
that need no second implementation - what a row's outputs hold around n_seg, float as one rounding of the double, the plane stride,
independence of the rows, the bound on the table queries, and the geometry of a cube's planes."""
import numpy as np
import pytest

from tests import cube_corridor_harness as ch


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("cube_corridor_cpp"))


@pytest.fixture(scope="module")
def rows(harness):
    grid = ch.random_map(80, 0.08)
    paths = ch.random_paths(grid, 16, seed=4)
    xyz, n = ch.pack_paths(paths)
    return grid, paths, xyz, n, ch.corridors(harness, grid, xyz, n, seg_capacity=40)


def test_outputs_around_n_seg(rows):
    grid, paths, xyz, n, r = rows
    assert (r["rtn"] == ch.OK).all() and r["n_seg"].min() >= 1 and r["n_seg"].max() > 3
    for b in range(len(paths)):
        k = r["n_seg"][b]
        assert (r["n_planes"][b, :k] == 6).all() and not r["n_planes"][b, k:].any()
        assert not r["planes"][b, k:].any() and not r["cube_idx"][b, k:].any() and not r["seeds"][b, k:].any()
        # the first polytope is seeded at the path's first voxel, and every seed's voxel lies in its own cube
        assert np.array_equal(np.rint((r["seeds"][b, 0] - ch.LOWER) / ch.RES - 0.5).astype(int), paths[b][0])
        vox = np.rint((r["seeds"][b, :k] - ch.LOWER) / ch.RES - 0.5).astype(int)
        assert (vox >= r["cube_idx"][b, :k, :3]).all() and (vox <= r["cube_idx"][b, :k, 3:]).all()


def test_planes_are_the_faces_of_the_cube_half_a_voxel_out(rows):
    grid, paths, xyz, n, r = rows
    for b in range(len(paths)):
        for k in range(r["n_seg"][b]):
            c, pl = r["cube_idx"][b, k], r["planes"][b, k]
            flat = (c[:3] == c[3:]).any()
            assert np.array_equal(pl[:, :3], [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1], [0, 1, 0], [1, 0, 0]])
            lo, hi = c[:3] * ch.RES + ch.LOWER, (c[3:] + 1) * ch.RES + ch.LOWER   # both kinds of cube end on voxel faces
            want = [lo[0], lo[1], lo[2], -hi[2], -hi[1], -hi[0]]
            assert np.allclose(pl[:, 3], want, rtol=0, atol=1e-12), (c, flat)
            ctr = r["centers"][b, k]
            assert (ctr > lo - 1e-12).all() and (ctr < hi + 1e-12).all()


def test_float_is_the_rounded_double_and_the_stride_is_the_callers(harness, rows):
    grid, paths, xyz, n, r = rows
    f = ch.corridors(harness, grid, xyz, n, seg_capacity=40, dtype=np.float32)
    for key in ("planes", "seeds", "centers"):
        assert f[key].dtype == np.float32 and np.array_equal(f[key].view(np.int32), r[key].astype(np.float32).view(np.int32)), key
    for key in ("n_seg", "n_planes", "cube_idx", "rtn"):
        assert np.array_equal(f[key], r[key])
    wide = ch.corridors(harness, grid, xyz, n, seg_capacity=40, p_max=9)
    assert np.array_equal(wide["planes"][:, :, :6], r["planes"]) and not wide["planes"][:, :, 6:].any()


def test_rows_are_independent_and_queries_bounded(harness, rows):
    grid, paths, xyz, n, r = rows
    perm = np.random.default_rng(0).permutation(len(paths))
    p = ch.corridors(harness, grid, xyz[perm], n[perm], seg_capacity=40)
    for key in ("n_seg", "n_planes", "planes", "seeds", "centers", "cube_idx", "rtn"):
        assert np.array_equal(p[key], r[key][perm]), key
    assert r["queries"].max() <= 6 * (sum(ch.DIMS) + 1)
    one = ch.corridors(harness, grid, xyz, n, seg_capacity=40, itr=1)
    assert one["queries"].max() <= 6 and (one["cube_idx"][:, :, 3:] - one["cube_idx"][:, :, :3]).max() <= 2


def test_path_length_codes(harness):
    grid = ch.crafted_map()
    xyz, n = ch.pack_paths([ch.line([20, 2, 2], [22, 2, 2])] * 4, cap=8)
    n[:] = [3, 0, -2, 9]   # good, empty, negative, longer than path_capacity (an OVERFLOW row of the path stage)
    r = ch.corridors(harness, grid, xyz, n, seg_capacity=4)
    assert r["rtn"].tolist() == [ch.OK, ch.BAD_PATH, ch.BAD_PATH, ch.BAD_PATH] and r["n_seg"].tolist()[1:] == [0, 0, 0] and r["n_seg"][0] >= 1
