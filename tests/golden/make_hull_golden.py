"""Golden vectors for the hull -> planes step from the REFERENCE'S OWN convex hull (global_planner/third_party/quickhull,
built from its sources into oracle/_ref/libquickhull_ref.so): for the 12 clusters of cluster_polygon_48.npz and four
flat ones, the vertex buffer and the triangles getConvexHull(points, true, false) returns for the point set
getConvexPoly builds (poly_utils.cpp:301-389); hull_quickhull_live_10.npz: the same for ten clusters the restated
polygonGeneration grows on a seeded random map (tests/test_hull.py).  Needs oracle/_ref (the reference's sources, oracle/Makefile):
    python tests/golden/make_hull_golden.py
hull_shapes.npz: the ORACLE'S answer (oracle/hull_ref.c) for every shape of tests/hull_shape_lib.py - large extents, voxel
shells, flat discs -, so that its slow runs (the larger shells) never happen inside a test; where oracle/_ref is
built every full-dimensional shape is pinned against the reference's quickhull first.  Needs no oracle/_ref:
    python tests/golden/make_hull_golden.py shapes
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from oracle import clusterapi, hullapi  # noqa: E402
from tests import hull_shape_lib as shapes  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def flat_clusters():
    return [np.array([[4, 4, 5]]), np.array([[x, y, 5] for x in range(3, 9) for y in range(4, 7)]),
            np.array([[3, y, z] for y in range(2, 5) for z in range(1, 7) if y + z != 3]),
            np.array([[x, 4, 5] for x in range(2, 7)])]


def main():
    hullapi.build()
    g = np.load(os.path.join(HERE, "cluster_polygon_48.npz"))
    off = np.concatenate([[0], np.cumsum(g["cluster_num"])])
    clusters = [g["cluster_xyz"][off[i]:off[i + 1]] for i in range(len(g["cluster_num"]))] + flat_clusters()
    out = dict(n=len(clusters))
    for i, cl in enumerate(clusters):
        deg = int(any(len(set(cl[:, a])) == 1 for a in range(3)))
        pts = hullapi.lattice_points(cl, deg)
        vb, tri = hullapi.reference_quickhull(pts.astype(np.float64))
        vbq = np.rint(vb).astype(np.int32)
        assert np.abs(vb - vbq).max() == 0
        out["cluster_%d" % i] = cl.astype(np.int32)
        out["deg_%d" % i] = deg
        out["qh_vertices_%d" % i] = vbq
        out["qh_triangles_%d" % i] = tri.astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "hull_quickhull_16.npz"), **out)
    print("wrote", len(clusters), "clusters")
    write_live_clusters()
    write_shapes()


def live_clusters(n=10):
    """The clusters of tests/test_hull.py's seeded random map, with the reference's quickhull of their point sets."""
    rng = np.random.default_rng(3)
    grid = (rng.random((90, 90, 28)) < 0.006).astype(np.uint8)
    out = dict(n=n)
    done = 0
    while done < n:
        seed = [int(rng.integers(15, 75)), int(rng.integers(15, 75)), int(rng.integers(5, 23))]
        if grid[tuple(seed)]:
            continue
        cl = clusterapi.polygon_generation(grid, seed)[1]
        deg = hullapi.hull_planes(cl, 0.2, np.array([-12.0, -12.0, 0.0]))["degenerate"]
        vb, tri = hullapi.reference_quickhull(hullapi.lattice_points(cl, deg).astype(np.float64))
        vbq = np.rint(vb).astype(np.int32)
        assert np.abs(vb - vbq).max() == 0
        out["cluster_%d" % done] = cl.astype(np.int32)
        out["deg_%d" % done] = int(deg)
        out["qh_vertices_%d" % done] = vbq
        out["qh_triangles_%d" % done] = tri.astype(np.int32)
        done += 1
    return out


def write_live_clusters():
    hullapi.build()
    assert hullapi.ref_lib() is not None, "build oracle/_ref first (make -C oracle _ref)"
    np.savez_compressed(os.path.join(HERE, "hull_quickhull_live_10.npz"), **live_clusters())


def write_shapes():
    hullapi.build()
    out = {}
    for name in shapes.SHAPES:
        cl = shapes.build(name)
        r = hullapi.hull_planes(cl, shapes.RES, shapes.LOWER, plane_cap=shapes.PLANE_CAP, vert_cap=shapes.VERT_CAP)
        assert r["rc"] in (0, 3), (name, r["rc"])
        if r["rc"] == 0 and hullapi.ref_lib() is not None:
            hullapi.check_against_quickhull(hullapi.lattice_points(cl, r["degenerate"]), r["plane_int"], r["vert_q"])
        out["%s/n" % name] = len(cl)
        for k in ("plane_int", "planes", "vert_q", "vertices", "center", "degenerate", "rc"):
            out["%s/%s" % (name, k)] = r[k]
        print("%-14s n %6d rc %d planes %4d corners %4d" % (name, len(cl), r["rc"], r["n_planes"], r["n_vertices"]), flush=True)
    np.savez_compressed(os.path.join(HERE, "hull_shapes.npz"), **out)


if __name__ == "__main__":
    write_shapes() if sys.argv[1:] == ["shapes"] else main()
