"""What is resident on a cluster handle after each event of DESIGN.md 6.22, asked through the public Python API alone: one handle
on a 12 x 10 x 8 map is driven through the table's rows in one sequence, and after every row each product is asked whether it
serves - with the words of the refusal where it does not.  The products and who asks: the map (get_map), the distance field
(plan_clearance, grid_paths_clear and cube_corridors_clear with min_d2 = 2, the last with info[0]: 1 when it had to build its floor
table), the free-space labels (free_components, reachable), the scan grid (scan_grid) and the resident clusters
(hull_planes(batch=...)).  No device error is provoked: the rows that lose a product are covered on the CPU
(tests/test_resident_state_cpp.py)."""
import numpy as np
import pytest

from direct_amd import abi, cluster, solver

pytestmark = pytest.mark.gpu

DIMS = (12, 10, 8)
LOWER, RES = (0.0, 0.0, 0.0), 1.0
SERVES = "serves"
NO_MAP = "the handle has no map"
NO_FIELD = "no valid distance field: call direct_cluster_distance_field after the map changes"
ABOVE_CAP = "min_d2 or n_penalty above the cap2 the distance field was built with"
STALE = "no valid free components: call direct_cluster_free_components after the map or the distance field changes"
OTHER_FLOOR = "min_d2 differs from the floor the free components were built with"
NO_SCAN = "the handle has no scan grid"
NO_CLUSTERS = "no resident clusters for this batch"
SEEDS = np.array([[2, 2, 2], [9, 7, 5]], np.int32)
# a straight row of voxels in front of the wall, in the layout of the grid-path outputs: what the corridor calls walk
ROW = np.zeros((1, 8, 3), np.int32)
ROW[0, :4] = [[1, 4, 3], [2, 4, 3], [3, 4, 3], [4, 4, 3]]
ROW_LEN = np.array([4], np.int32)
# one quintic piece standing still in voxel (3, 3, 3): x = y = z, so the coefficient layout does not matter
PLAN = dict(n_seg=np.array([1], np.int32), T=np.ones((1, 1)), bez=np.full((1, 1, 18), 3.5))


def wall():
    """the wall x == 6 with a door y in [3, 6], through every z"""
    g = np.zeros(DIMS, np.uint8)
    g[6, :, :] = 1
    g[6, 3:7, :] = 0
    return g


def centres(voxels):
    return (np.asarray(voxels, np.float64) + 0.5).astype(np.float32)


def ask(call):
    """-> (SERVES, the call's result) or (the words of the refusal, None)"""
    try:
        return SERVES, call()
    except solver.DirectError as e:
        assert e.status == abi.DIRECT_ERR_INVALID, e
        return str(e).split(": ", 1)[1], None


def refused(call, words):
    said, _ = ask(call)
    assert said == words, said


class Want:
    """what the next look expects: per product SERVES or the refusal's words; built: cube_corridors_clear's info[0]; floor: the
    floor the labels were built with, which reachable is asked with"""

    def __init__(self):
        self.map = self.field = self.labels = NO_MAP
        self.scan, self.clusters = NO_SCAN, 0
        self.built, self.floor = 1, 0


def look(g, w, row):
    said = {}
    said["map"], _ = ask(g.get_map)
    said["plan_clearance"], _ = ask(lambda: g.plan_clearance(map_lower=LOWER, resolution=RES, **PLAN))
    said["grid_paths_clear"], _ = ask(lambda: g.grid_paths_clear([[1, 1, 1]], [[10, 8, 6]], min_d2=2, path_capacity=64))
    said["cube_corridors_clear"], cubes = ask(lambda: g.cube_corridors_clear(ROW, ROW_LEN, LOWER, RES, 2, seg_capacity=8))
    said["free_components"], _ = ask(g.free_components)
    said["reachable"], _ = ask(lambda: g.reachable([[1, 1, 1]], [[10, 8, 6]], min_d2=w.floor))
    said["scan_grid"], _ = ask(g.scan_grid)
    said["hull_planes"] = [ask(lambda: g.hull_planes(RES, LOWER, batch=b, want=("center",)))[0].split(":")[0] for b in (1, 2)]
    want = {"map": w.map, "plan_clearance": w.field, "grid_paths_clear": w.field, "cube_corridors_clear": w.field,
            "free_components": w.labels, "reachable": w.labels, "scan_grid": w.scan,
            "hull_planes": [SERVES if b <= w.clusters else NO_CLUSTERS for b in (1, 2)]}
    assert said == want, (row, said, want)
    if w.field == SERVES:
        assert int(cubes["info"][0]) == w.built, (row, cubes["info"], w.built)
        w.built = 0  # its table is resident now
    if w.labels == SERVES:
        assert g.free_components_floor() == w.floor, row
        refused(lambda: g.reachable([[1, 1, 1]], [[10, 8, 6]], min_d2=w.floor + 3), OTHER_FLOOR)


def test_every_row_of_the_event_table(built):
    g = cluster.ClusterGenerator(DIMS, max_batch=2, cluster_capacity=256, candidate_capacity=64)
    w = Want()
    look(g, w, "a new handle")

    g.set_map(wall())
    w.map, w.field, w.labels = SERVES, NO_FIELD, STALE
    look(g, w, "set_map")

    g.build_distance_field()
    w.field = SERVES
    look(g, w, "distance_field")
    look(g, w, "distance_field, asked again: the floor table is reused")

    g.build_free_components(2)
    w.labels, w.floor = SERVES, 2
    look(g, w, "free_components with a floor")

    g.polygon_generation(SEEDS, itr_cluster_max=2, fetch_clusters=False)
    w.clusters = 2
    look(g, w, "polygon_generation_batch")

    refused(lambda: g.build_distance_field(cap_vox=-1), "cap_vox outside [0, 1024]")
    w.labels = STALE  # built with a floor: the refused call counts too; the field itself and its floor tables stay
    look(g, w, "distance_field, refused, labels with a floor")

    g.build_free_components(0)
    w.labels, w.floor = SERVES, 0
    look(g, w, "free_components without a floor")
    refused(lambda: g.build_distance_field(cap_vox=-1), "cap_vox outside [0, 1024]")
    look(g, w, "distance_field, refused, labels without a floor")

    g.build_distance_field(cap_vox=1)  # cap2 = 1: a field, but a floor of 2 cannot be told from its cap
    assert ask(lambda: g.plan_clearance(map_lower=LOWER, resolution=RES, **PLAN))[0] == SERVES
    for call in (lambda: g.grid_paths_clear([[1, 1, 1]], [[10, 8, 6]], min_d2=2, path_capacity=64),
                 lambda: g.cube_corridors_clear(ROW, ROW_LEN, LOWER, RES, 2, seg_capacity=8),
                 lambda: g.build_free_components(2)):
        refused(call, ABOVE_CAP)
    assert ask(g.free_components)[0] == SERVES  # the labels without a floor outlive a new field, and a refused build of their own

    g.build_distance_field()
    w.field, w.built = SERVES, 1  # a new serial: every floor table misses
    look(g, w, "distance_field, a second field")
    # the two floor slots: a miss into the empty one, hits, a miss into the least recently used
    info = lambda floor: int(g.cube_corridors_clear(ROW, ROW_LEN, LOWER, RES, floor, seg_capacity=8)["info"][0])
    assert [info(f) for f in (4, 2, 4, 2, 5, 2, 4)] == [1, 0, 0, 0, 1, 0, 1]  # 5 evicted 4, then 4 evicted 5
    look(g, w, "the floor slots")

    refused(lambda: g.set_map_from_cloud(centres([[6, 0, 0]]), LOWER, -1.0, 0.0), "resolution must be finite and positive")
    w.field, w.labels = NO_FIELD, STALE  # the refused call counts as a map edit; the map's bytes are still there
    look(g, w, "map_from_cloud, refused")
    assert np.array_equal(g.get_map(), wall())

    g.build_distance_field()
    g.build_free_components(2)
    w.field, w.built, w.labels, w.floor = SERVES, 1, SERVES, 2
    look(g, w, "field and labels rebuilt")

    g.set_map_from_cloud(centres([[6, y, z] for y in (0, 1, 2, 7, 8, 9) for z in range(8)]), LOWER, RES, 0.0)
    assert np.array_equal(g.get_map(), wall())
    w.field, w.labels = NO_FIELD, STALE
    look(g, w, "map_from_cloud")

    g.build_distance_field()
    g.build_free_components(2)
    w.field, w.built, w.labels = SERVES, 1, SERVES
    look(g, w, "field and labels rebuilt after the cloud")

    origin = (1.5, 1.5, 1.5)
    refused(lambda: g.integrate_scan(centres([[3, 1, 1]]), origin, LOWER, RES, -1.0), "max_range must be finite and positive")
    look(g, w, "map_integrate_scan, refused")

    st = g.integrate_scan(np.zeros((0, 3), np.float32), origin, LOWER, RES, 20.0, mode="adopt")
    assert st["set"] + st["cleared"] == 0
    w.scan = SERVES
    look(g, w, "map_integrate_scan, unchanged")  # field, floor table (built stays 0) and labels kept
    assert np.array_equal(g.scan_grid(), wall())

    st = g.integrate_scan(centres([[3, 1, 1]]), origin, LOWER, RES, 20.0)
    assert st["set"] == 1 and st["cleared"] == 0
    w.field, w.labels = NO_FIELD, STALE
    look(g, w, "map_integrate_scan, changed")
    assert g.get_map()[3, 1, 1] == 1

    g.build_distance_field()
    g.build_free_components(0)
    w.field, w.built, w.labels, w.floor = SERVES, 1, SERVES, 0
    look(g, w, "field and labels rebuilt after the scan")

    # the calls that write the cluster storage; one that is refused leaves it alone
    again = lambda: g.polygon_generation(SEEDS, itr_cluster_max=2, fetch_clusters=False)
    refused(lambda: g.polygon_generation(np.zeros((3, 3), np.int32), fetch_clusters=False), "batch exceeds the handle's max_batch")
    look(g, w, "polygon_generation_batch, refused")
    g.polygon_generation(SEEDS[:1], itr_cluster_max=2, fetch_clusters=False)
    w.clusters = 1
    look(g, w, "polygon_generation_batch of one seed")
    g.convex_test(np.zeros(DIMS, np.uint8), [[1, 1, 1]], [[2, 2, 2]])
    w.clusters = 0
    look(g, w, "convex_test")
    again()
    w.clusters = 2
    look(g, w, "polygon_generation_batch again")
    cube = np.array([[x, y, z] for x in (1, 2) for y in (1, 2) for z in (1, 2)], np.int32)
    g.hull_planes(RES, LOWER, clusters=[cube], want=("center",))
    w.clusters = 0
    look(g, w, "hull_planes_batch with caller voxels")
    again()
    g.cluster_corridors(ROW, ROW_LEN, LOWER, RES, itr_cluster_max=2, seg_capacity=8, p_max=32)
    look(g, w, "corridor_batch")

    again()
    g.set_map(wall())
    w.field, w.labels, w.clusters = NO_FIELD, STALE, 2  # the scan grid and the clusters are not the map's
    look(g, w, "set_map again")
    g.close()
