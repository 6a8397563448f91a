"""direct_amd/csrc/dist_field_math.h compiled by g++ against the NumPy brute force of tests/dist_field_harness.py: the stored field
of direct_cluster_distance_field, integer for integer, and its stats.  No GPU."""
import numpy as np
import pytest

from tests import dist_field_harness as dh


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("dist_field"))


@pytest.fixture(scope="module")
def grids():
    """(name, grid, uncapped brute force) once for all tests"""
    return [(name, g, dh.brute_d2(g)) for name, g in dh.shared_grids()]


def test_the_two_brute_forces_agree(grids):
    """wherever the pair-by-pair minimum can run, the line-by-line one gives the same integers"""
    both = 0
    for name, g, want in grids:
        if float(np.count_nonzero(g == 1)) * g.size <= dh.PAIR_LIMIT:
            assert np.array_equal(dh.brute_d2(g, force="linewise"), want), name
            both += 1
    assert both >= 20


def test_brute_force_on_a_grid_worked_by_hand():
    g = np.zeros((4, 3, 2), np.uint8)
    g[0, 0, 0] = g[3, 2, 1] = 1
    d2 = dh.brute_d2(g)
    assert d2[0, 0, 0] == 0 and d2[3, 2, 1] == 0 and d2[1, 0, 0] == 1 and d2[1, 1, 1] == 3 and d2[2, 2, 0] == 2 and d2[3, 0, 0] == 5
    assert dh.brute_d2(g, 1)[1, 1, 1] == 1 and dh.brute_d2(g, 4)[3, 0, 0] == 5
    assert (dh.brute_d2(np.zeros((2, 2, 2), np.uint8)) == dh.NONE).all() and (dh.brute_d2(np.zeros((2, 2, 2), np.uint8), 4) == 16).all()


@pytest.mark.parametrize("cap_vox", dh.CAPS)
def test_header_equals_brute_force(harness, grids, cap_vox):
    for name, g, exact in grids:
        want = np.minimum(exact, dh.cap2_of(cap_vox)).astype(np.int32)
        got, stats, _ms = dh.run_field(harness, g, cap_vox)
        bad = np.argwhere(got != want)
        assert not len(bad), f"{name} cap {cap_vox}: {len(bad)} voxels differ, first {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        assert stats == dh.field_stats(want, cap_vox), f"{name} cap {cap_vox}"


def test_the_grids_cover_what_they_should(grids):
    by_name = {name: (g, d2) for name, g, d2 in grids}
    assert (by_name["65x64x63 empty"][1] == dh.NONE).all() and (by_name["65x64x63 100%"][1] == 0).all()
    g, d2 = by_name["65x64x63 corner"]
    assert g.sum() == 1 and d2[0, 63, 0] == 64 ** 2 + 63 ** 2 + 62 ** 2 and d2.max() == d2[0, 63, 0]
    assert by_name["2x3x261 corner"][1][0, 2, 0] == 1 + 4 + 260 ** 2
    assert by_name["shared_map"][0].shape == (40, 36, 12) and 0 < by_name["shared_map"][1].max() < dh.NONE
