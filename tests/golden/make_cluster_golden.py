"""Generates tests/golden/cluster_*.npz: vectors for the corridor-cluster path produced with the REFERENCE'S OWN
serialConvexTest (oracle/_ref/libcluster_engine_ref.so, compiled from
/root/reference/polyhedron_generator/src/cluster_engine_cpu.cpp by `make -C oracle _ref`).

  cluster_convex_*.npz  one clustering round frozen right before its convex tests: map, inside flags, candidates,
                        cluster -> can_clu[i] = serialConvexTest(candidate i, whole cluster), can_can (packed lower
                        triangle) = serialConvexTest(candidate i, {candidate j}), accept = the sequential loop's
                        decisions.  Every value comes from the reference function.
  cluster_polygon_*.npz polygonGeneration for a few seeds: the loops around serialConvexTest are the restatement
                        of oracle/cluster_ref.c (cluster_server_cpu.cpp needs ROS headers and cannot be built),
                        run with the reference function plugged in.
  cluster_convex_random_12.npz  twelve seeded random scenes (map, inside box, 60 candidates, a 6-voxel cluster) and
                        serialConvexTest of every candidate against the cluster.
  cluster_shell_classes.npz  the scenes of tests/cluster_shell_lib.py (a box with one stopper per face and obstacles on the
                        edge rows of its first shell: 4095 ... 18000 candidates in the first round), two clustering rounds each
                        through the restated loops with the reference function plugged in: per scene the generator's
                        parameters, seed, vertex_idx, iters, the cluster size after the surface and after every round, every
                        round's candidate count, the per-range report, the cluster and the SHA-256 of its int32 bytes.
Run from the repo root in the build container: python tests/golden/make_cluster_golden.py
(`python tests/golden/make_cluster_golden.py shell` writes cluster_shell_classes.npz alone)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from direct_amd import problems  # noqa: E402
from oracle import clusterapi as ca  # noqa: E402
from tests import cluster_shell_lib as shell  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def convex_case(grid, seed, rounds):
    """State of the clustering loop of `seed` after `rounds` completed rounds, frozen before the next convex tests."""
    R = ca.ref_lib()
    dims = grid.shape
    v, surf, _, _ = ca.polygon_generation(grid, seed, itr_cluster_max=0)
    use, inside = ca.cube_state(grid, v)
    invalid = np.zeros(dims, np.uint8)
    cluster, active = surf.copy(), surf.copy()
    for r in range(rounds + 1):
        cand = ca.candidates(grid, use, invalid, inside, active)
        n = len(cand)
        can_clu = ca.serial_convex_test(R, "ref_serial_convex_test", cand, cluster, inside, grid, dims)
        can_can = np.zeros(n * (n - 1) // 2, np.uint8)
        for i in range(n):
            for j in range(i):
                can_can[i * (i - 1) // 2 + j] = ca.serial_convex_test(R, "ref_serial_convex_test", cand[i:i + 1], cand[j:j + 1],
                                                                       inside, grid, dims)[0]
        accept = ca.accept_sequential(can_clu, can_can)
        if r == rounds:
            return dict(grid=grid, inside=inside, cand=cand, cluster=cluster, can_clu=can_clu, can_can=can_can, accept=accept,
                        vertex_idx=v)
        for i in range(n):
            if not accept[i]:
                invalid[tuple(cand[i])] = 1
        cluster = np.concatenate([cluster, cand[accept == 1]])
        active = cand[accept == 1]


def random_scenes(n=12):
    """Seeded random scenes that exercise both outcomes of serialConvexTest, with the reference's answers."""
    R = ca.ref_lib()
    rng = np.random.default_rng(3)
    out = dict(n=n)
    for trial in range(n):
        dims = (int(rng.integers(10, 40)), int(rng.integers(10, 40)), int(rng.integers(5, 16)))
        grid = (rng.random(dims) < rng.uniform(0.002, 0.03)).astype(np.uint8)
        inside = np.zeros(dims, np.uint8)
        lo = [int(rng.integers(1, d // 2)) for d in dims]
        hi = [int(rng.integers(d // 2, d - 1)) for d in dims]
        inside[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
        cand = np.stack([rng.integers(0, d, 60) for d in dims], 1).astype(np.int32)
        clu = np.stack([rng.integers(0, d, 6) for d in dims], 1).astype(np.int32)
        out.update({"grid_%d" % trial: grid, "inside_%d" % trial: inside, "cand_%d" % trial: cand, "cluster_%d" % trial: clu,
                    "can_clu_%d" % trial: ca.serial_convex_test(R, "ref_serial_convex_test", cand, clu, inside, grid, dims)})
    return out


def write_random_scenes():
    assert ca.ref_lib() is not None, "build oracle/_ref first (make -C oracle _ref)"
    np.savez_compressed(os.path.join(OUT, "cluster_convex_random_12.npz"), **random_scenes())


def write_shell_classes():
    """cluster_shell_classes.npz; every scene meets the conditions on the inputs and has the candidate count it promises."""
    reference = ca.ref_lib() is not None
    names = shell.scene_names()
    res = shell.run_scenes(names, reference=reference)
    out = dict(names=np.array(names), reference=np.array(bool(reference)))
    for n in names:
        sc, r = shell.scene(n), res[n]
        bad = shell.unmet_conditions(r)
        print(shell.format_report(n, r))
        assert not bad, (n, bad)
        assert r["n_cand"][0] == sc["expect_candidates"], (n, r["n_cand"], sc["expect_candidates"])
        out.update({n + "_cube": np.array(sc["cube"], np.int32), n + "_n_shell": np.int32(sc["n_shell"]),
                    n + "_n_outer": np.int32(sc["n_outer"]), n + "_seed": sc["seed"], n + "_vertex_idx": r["vertex_idx"],
                    n + "_iters": np.int32(r["iters"]), n + "_sizes": r["sizes"], n + "_n_cand": r["n_cand"],
                    n + "_report": np.array([[q[c] for c in shell.REPORT_COLUMNS] for q in r["report"]], np.int32),
                    n + "_sha256": np.array(shell.cluster_digest(r["cluster"])), n + "_cluster": r["cluster"]})
    path = os.path.join(OUT, "cluster_shell_classes.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, "past the size limit of a committed file: store digests for the boundary scenes"
    print("cluster_shell_classes.npz: %d bytes" % os.path.getsize(path))


def main():
    assert ca.ref_lib() is not None, "build oracle/_ref first (make -C oracle _ref)"
    grid, seeds = problems.make_voxel_map((48, 48, 16), seed=11, n_pillars=22, n_boxes=10, n_rings=2)
    for name, seed, rounds in (("a", seeds[0], 0), ("b", seeds[3], 1)):
        c = convex_case(grid, seed, rounds)
        assert 0 < c["accept"].sum() < len(c["accept"]), (name, c["accept"].sum(), len(c["accept"]))
        np.savez_compressed(os.path.join(OUT, "cluster_convex_%s.npz" % name), seed=seed, **c)
        print(name, "candidates", len(c["cand"]), "cluster", len(c["cluster"]), "can_clu", int(c["can_clu"].sum()),
              "accept", int(c["accept"].sum()), "blocked pairs", int((c["can_can"] == 0).sum()))
    ca.use_reference_convex_test(True)
    sel = seeds[:12]
    vs, cls, its = [], [], []
    for s in sel:
        v, cl, it, rc = ca.polygon_generation(grid, s, itr_inflate_max=1000, itr_cluster_max=50)
        assert rc == 0
        vs.append(v); cls.append(cl); its.append(it)
    ca.use_reference_convex_test(False)
    num = np.array([len(c) for c in cls], np.int32)
    np.savez_compressed(os.path.join(OUT, "cluster_polygon_48.npz"), grid=grid, seeds=sel, vertex_idx=np.array(vs),
                        cluster_num=num, cluster_xyz=np.concatenate(cls), iters=np.array(its, np.int32))
    print("polygon: clusters", num.tolist(), "iters", its)
    write_random_scenes()
    write_shell_classes()


if __name__ == "__main__":
    if sys.argv[1:] == ["shell"]:
        write_shell_classes()
    else:
        main()
