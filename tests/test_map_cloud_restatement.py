"""The map from a point cloud (include/direct_cluster.h, "the map from a point cloud") on the CPU:
direct_amd/csrc/map_cloud_math.h compiled by g++ as a program (tests/map_cloud_harness.py) against a NumPy restatement of the
reference's rcvPointCloudCallBack written from the reference's text, bit for bit (maps are bytes: there are no tolerances), for
both border conventions, both strides and the three margins; the product form against the literal loop nest; and checks that the
inputs CAN catch the mistakes they are there for."""
import os

import numpy as np
import pytest

from tests import map_cloud_harness as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return mh.build(tmp_path_factory.mktemp("map_cloud"))


@pytest.fixture(scope="module")
def clouds():
    return mh.clouds()


def test_steps():
    """TRP:537-538: 0.0 -> (0, 1), 0.25 -> (2, 1), 0.45 -> (3, 1) at 0.15 m; z has at least one step and half of s beyond 2"""
    assert [mh.steps(m, mh.RES) for m in mh.MARGINS] == [(0, 1), (2, 1), (3, 1)]
    assert mh.steps(0.9, 0.15) == (6, 3) and mh.steps(0.375, 0.15) == (3, 1) and mh.steps(0.1, 0.2) == (1, 1)


@pytest.mark.parametrize("border", (mh.CLAMP, mh.DROP), ids=("clamp", "drop"))
@pytest.mark.parametrize("margin", mh.MARGINS)
def test_header_program_equals_the_restatement(harness, clouds, margin, border):
    for name, pts in clouds.items():
        want, wstats = mh.restate(pts, margin, border)
        for stride in (3, 4):
            got, gstats, _ = mh.run(harness, pts if stride == 3 else mh.with_stride4(pts), margin, border)
            assert np.array_equal(got, want), (name, stride, int((got != want).sum()))
            assert np.array_equal(gstats, wstats), (name, stride, gstats, wstats)
        assert wstats[3] > 0


@pytest.mark.parametrize("border", (mh.CLAMP, mh.DROP), ids=("clamp", "drop"))
@pytest.mark.parametrize("margin", mh.MARGINS)
def test_product_form_equals_the_triple_loop(clouds, margin, border):
    for name in ("faces", "borders", "nonfinite"):
        want, wstats = mh.triple_loop(clouds[name], margin, border)
        got, gstats = mh.restate(clouds[name], margin, border)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert np.array_equal(gstats, wstats), (name, gstats, wstats)


def test_add_onto_a_map(harness, clouds):
    pts = clouds["random"]
    whole, _ = mh.restate(pts, 0.25, mh.CLAMP)
    half, _ = mh.restate(pts[:1000], 0.25, mh.CLAMP)
    both, stats = mh.restate(pts[1000:], 0.25, mh.CLAMP, base=half)
    assert np.array_equal(both, whole) and stats[0] == 1000 and stats[3] == whole.sum()
    got, gstats, _ = mh.run(harness, pts[1000:], 0.25, mh.CLAMP, base=half)
    assert np.array_equal(got, whole) and np.array_equal(gstats, stats)


def test_inflation_acts_on_coordinates_not_on_voxels(clouds):
    """the face points tell the reference's map from a box dilation of each point's own voxel"""
    want, _ = mh.restate(clouds["faces"], 0.25, mh.CLAMP)
    box = mh.dilate_base_voxel(clouds["faces"], 0.25)
    differ = int((want != box).sum())
    print("coordinate-wise inflation and voxel-wise dilation differ in %d voxels for %d face points" % (differ, len(clouds["faces"])))
    assert differ >= 1
    # ... and points in the open interior of their voxels do not: the difference is the faces', not the dilation helper's
    inner = (mh.LOWER + (np.array([[5, 6, 3], [14, 17, 8], [23, 28, 3]]) + 0.5) * mh.RES).astype(np.float32)
    assert np.array_equal(mh.restate(inner, 0.25, mh.CLAMP)[0], mh.dilate_base_voxel(inner, 0.25))


def test_the_two_border_conventions_differ(clouds):
    for margin in mh.MARGINS:
        c, cs = mh.restate(clouds["borders"], margin, mh.CLAMP)
        d, ds = mh.restate(clouds["borders"], margin, mh.DROP)
        assert (c != d).any() and cs[2] == 0 and ds[2] > 0
        assert (d <= c).all()  # what drop keeps, clamp keeps in the same voxel


def test_the_gap_below_the_upper_corner_is_dropped(harness):
    """a coordinate in [size * resolution + lower, upper) passes the reference's range test and indexes one past its array"""
    z = np.float32(mh.LOWER[2] + mh.DIMS[2] * mh.RES + 0.02)
    assert mh.LOWER[2] + mh.DIMS[2] * mh.RES <= float(z) < mh.UPPER[2]
    pts = np.array([[0.01, 0.02, z]], np.float32)
    got, stats, _ = mh.run(harness, pts, 0.0, mh.DROP)
    want, wstats = mh.restate(pts, 0.0, mh.DROP)
    assert np.array_equal(got, want) and np.array_equal(stats, wstats)
    assert stats[2] == 2 and stats[3] == 1 and got[20, 18, 11] == 1  # z and z + res dropped, z - res is the top voxel


def test_margin_zero_still_inflates_z(harness):
    """map_margin = 0.0, the launch file's value: nothing beside the point's voxel, one voxel above and one below"""
    pts = (mh.LOWER + (np.array([[10, 11, 5]]) + 0.5) * mh.RES).astype(np.float32)
    for grid in (mh.restate(pts, 0.0, mh.CLAMP)[0], mh.run(harness, pts, 0.0, mh.CLAMP)[0]):
        assert np.array_equal(np.argwhere(grid == 1), [[10, 11, 4], [10, 11, 5], [10, 11, 6]])


def test_nonfinite_rows_are_skipped_and_counted(harness, clouds):
    pts = clouds["nonfinite"]
    fin = np.isfinite(pts).all(axis=1)
    assert (~fin).sum() == 5
    for border in (mh.CLAMP, mh.DROP):
        got, stats, _ = mh.run(harness, pts, 0.25, border)
        assert stats[0] == len(pts) and stats[1] == 5
        assert np.array_equal(got, mh.run(harness, pts[fin], 0.25, border)[0])
    # 1e30 is finite: clamp marks the border, drop discards
    far = np.array([[1e30, 0.0, 0.5]], np.float32)
    assert mh.run(harness, far, 0.0, mh.CLAMP)[0][39].sum() == 3 and mh.run(harness, far, 0.0, mh.DROP)[1][3] == 0


def test_header_names_its_contraction_rule_and_the_abi_declares_the_calls():
    text = open(os.path.join(ROOT, "direct_amd", "csrc", "map_cloud_math.h")).read()
    assert "fp contract(off)" in text and "namespace mapcloud" in text
    from direct_amd import cluster
    assert {"direct_cluster_map_from_cloud", "direct_cluster_get_map"} <= set(cluster.EXPORTS)
    head = open(os.path.join(ROOT, "include", "direct_cluster.h")).read()
    for word in ("DIRECT_MAP_BORDER_CLAMP", "DIRECT_MAP_BORDER_DROP", "DIRECT_MAP_REPLACE", "DIRECT_MAP_ADD", "direct_map_cloud_t"):
        assert word in head
