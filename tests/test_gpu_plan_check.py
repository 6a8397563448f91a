"""direct_cluster_plan_check_batch on the GPU against the NumPy restatement of tests/plan_check_harness.py, which judges every leaf:
equal outputs, integer for integer and bit for bit of t_free.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from direct_amd import abi, cluster
from tests import map_cloud_harness as mh
from tests import plan_check_harness as ph

pytestmark = pytest.mark.gpu
OUTS = ("status", "verdict", "t_free", "first", "hit_box", "seg_first")


@pytest.fixture(scope="module")
def grid():
    return ph.shared_map()


@pytest.fixture(scope="module")
def gen(built, grid):
    g = cluster.ClusterGenerator(mh.DIMS, max_batch=4, cluster_capacity=2048, candidate_capacity=512)
    g.set_map(grid)
    yield g
    g.close()


@pytest.fixture(scope="module")
def inputs():
    return ph.shared_inputs()


def check(gen, inp, depth, margin=0.0, ob=False, use_t_from=True, device=False, count=False):
    """check_plans on an input dict of the harness (one of bez / poly), from host arrays or from device tensors -> NumPy outputs"""
    kind = "poly" if inp.get("poly") is not None else "bez"
    args = dict(n_seg=inp["n_seg"], T=inp["T"], t_from=inp.get("t_from") if use_t_from else None)
    args[kind] = inp[kind]
    if device:
        import torch
        args = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")) for k, v in args.items()}
    out = gen.check_plans(map_lower=ph.LOWER, resolution=ph.RES, depth=depth, margin=margin, outside_blocks=ob, count=count, **args)
    return {k: (v.cpu().numpy() if device and k in OUTS else v) for k, v in out.items()}


# every listed value of every option appears, each against the restatement of exactly its own options
COMBOS = (("bez", False, False, True, False, 0.0), ("poly", True, True, False, True, 0.2), ("bez", True, False, False, True, 0.0),
          ("poly", False, True, True, False, 0.2))


@pytest.mark.parametrize("depth", [0, 1, 5, 6, 7, 12])
def test_outputs_equal_the_restatement(gen, grid, inputs, depth):
    names = ("random7", "crafted", "invalid9") + (("long5",) if depth <= 7 else ())
    for name in names:
        for kind, f32, device, use_t_from, ob, margin in COMBOS:
            inp = ph.pick(inputs[name], kind)
            inp = ph.as_f32(inp) if f32 else inp
            want = ph.restate(inp, grid, depth, margin, ob, use_t_from)
            got = check(gen, inp, depth, margin, ob, use_t_from, device)
            ph.assert_same(got, want, f"{name} D={depth} {kind} f32={f32} device={device} t_from={use_t_from} outside={ob} margin={margin}")
    assert gen.last_ms() > 0.0


def test_depths_leave_work_for_the_deep_pass(gen, inputs):
    """the shared inputs do reach the second kernel: some slot is left unresolved at the larger depths"""
    assert check(gen, ph.pick(inputs["long5"], "bez"), 7, use_t_from=False, count=True)["unresolved"] > 0
    out = check(gen, ph.pick(inputs["long5"], "bez"), 0, use_t_from=False, count=True)
    assert out["unresolved"] == 0 and out["box_tests"] == int(inputs["long5"]["n_seg"].sum())


def rows_of(inp, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in inp.items()}


@pytest.mark.parametrize("name", ["crafted", "long5"])
def test_launch_shape(gen, inputs, name):
    """one call, two calls of halves and a permuted batch give identical rows"""
    inp = ph.pick(inputs[name], "poly")
    B = len(inp["n_seg"])
    whole = check(gen, inp, 7, ob=True)
    h = B // 2
    halves = [check(gen, rows_of(inp, slice(0, h)), 7, ob=True), check(gen, rows_of(inp, slice(h, B)), 7, ob=True)]
    perm = np.random.default_rng(5).permutation(B)
    shuffled = check(gen, rows_of(inp, perm), 7, ob=True)
    for k in OUTS:
        assert np.array_equal(np.concatenate([halves[0][k], halves[1][k]]), whole[k], equal_nan=True), k
        assert np.array_equal(shuffled[k], whole[k][perm], equal_nan=True), k


def test_the_table_is_current(built, grid, inputs):
    """check, add one point to the map on a free row's path, check again: that row is blocked and no other row changes; then an
    empty map frees every valid row"""
    g = cluster.ClusterGenerator(mh.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)
    g.set_map(grid)
    inp = ph.pick(inputs["crafted"], "bez")
    r = ph.CRAFTED.index("free")
    before = check(g, inp, ph.CRAFTED_DEPTH, use_t_from=False)
    assert before["verdict"][r] == 0
    point = np.array([[-1.7, ph.lane_y(0), ph.LANE_Z]], np.float32)     # inside segment 1 (x in [-2.1, -1.3]), in voxel x = 8, away from the joint at -2.1, which lies on a voxel face
    g.set_map_from_cloud(point, ph.LOWER, ph.RES, cloud_margin=0.0, add=True)
    now = g.get_map()
    after = check(g, inp, ph.CRAFTED_DEPTH, use_t_from=False)
    ph.assert_same(after, ph.restate(inp, now, ph.CRAFTED_DEPTH, use_t_from=False), "after ADD")
    assert after["verdict"][r] == 1 and after["first"][r][0] == 1 and 1.0 <= after["t_free"][r] < 2.0
    others = [b for b in range(len(ph.CRAFTED)) if b != r]
    for k in OUTS:
        assert np.array_equal(after[k][others], before[k][others]), k
    g.set_map_from_cloud(np.zeros((0, 3), np.float32), ph.LOWER, ph.RES, cloud_margin=0.0)
    empty = check(g, inp, ph.CRAFTED_DEPTH, use_t_from=False)
    assert (empty["status"] == 0).all() and (empty["verdict"] == 0).all() and (empty["first"] == -1).all()
    assert np.array_equal(empty["t_free"], inp["n_seg"].astype(np.float64))    # T = 1 per segment
    g.close()


def test_invalid_rows(gen, grid, inputs):
    inp = ph.pick(inputs["invalid9"], "bez")
    out = check(gen, inp, 6)
    bad = sorted(ph.INVALID_ROWS)
    good = [b for b in range(9) if b not in bad]
    assert (out["status"][bad] == -1).all() and (out["verdict"][bad] == cluster.PLAN_CHECK_INVALID).all() and (out["t_free"][bad] == 0).all()
    assert (out["first"][bad] == -1).all() and (out["hit_box"][bad] == -1).all() and (out["seg_first"][bad] == -1).all()
    alone = check(gen, rows_of(inp, good), 6)     # the valid rows' results do not depend on their neighbours
    for k in OUTS:
        assert np.array_equal(out[k][good], alone[k]), k
    assert (out["status"][good] == 0).all()


def raw_call(g, inp, outs=OUTS, **change):
    """the C call on host arrays with fields of the input struct replaced -> (status code, output arrays prefilled with 77)"""
    kind = "poly" if inp.get("poly") is not None else "bez"
    T, coef, n_seg = (np.ascontiguousarray(inp["T"], np.float64), np.ascontiguousarray(inp[kind], np.float64),
                      np.ascontiguousarray(inp["n_seg"], np.int32))
    B, N = T.shape
    par = cluster.PlanCheckIn(batch=B, n_seg_max=N, mem=abi.MEM_HOST, dtype=abi.F64, n_seg=n_seg.ctypes.data, T=T.ctypes.data,
                              map_lower=(C.c_double * 3)(*ph.LOWER), resolution=ph.RES, margin=0.0, depth=5, outside_blocks=0)
    setattr(par, kind, coef.ctypes.data)
    for k, v in change.items():
        setattr(par, k, v)
    arr = dict(status=np.full(B, 77, np.int32), verdict=np.full(B, 77, np.int32), t_free=np.full(B, 77.0), first=np.full((B, 2), 77, np.int32),
               hit_box=np.full((B, 6), 77, np.int32), seg_first=np.full((B, N), 77, np.int32))
    o = cluster.PlanCheckOut(**{k: arr[k].ctypes.data for k in outs})
    return cluster._lib().direct_cluster_plan_check_batch(g.h, C.addressof(par), C.addressof(o)), arr, (par, T, coef, n_seg)


NAN3, SOME = (C.c_double * 3)(0.0, float("nan"), 0.0), np.zeros(8)
# every single fault with the words of its refusal, as direct_cluster_last_error() gives them
FAULTS = [(dict(n_seg=None), b"null argument"), (dict(T=None), b"null argument"), (dict(batch=0), b"batch and n_seg_max must be positive"),
          (dict(batch=-1), b"batch and n_seg_max must be positive"), (dict(n_seg_max=0), b"batch and n_seg_max must be positive"),
          (dict(bez=None), b"exactly one of bez and poly"), (dict(poly=SOME.ctypes.data), b"exactly one of bez and poly"),
          (dict(mem=2), b"neither DIRECT_MEM_HOST"), (dict(dtype=2), b"dtype is neither"), (dict(depth=-1), b"depth outside"),
          (dict(depth=13), b"depth outside"), (dict(map_lower=NAN3), b"map_lower"), (dict(margin=-0.1), b"margin must be"),
          (dict(margin=float("nan")), b"margin must be"), (dict(resolution=0.0), b"resolution must be"), (dict(resolution=-1.0), b"resolution must be"),
          (dict(resolution=float("inf")), b"resolution must be"), (dict(resolution=float("nan")), b"resolution must be"),
          (dict(outside_blocks=2), b"outside_blocks")]


def test_invalid_arguments_launch_nothing(gen, inputs):
    inp = ph.pick(inputs["random7"], "bez")
    for change, _words in FAULTS:
        st, arr, _keep = raw_call(gen, inp, **change)
        assert st == abi.DIRECT_ERR_INVALID, change
        assert all((a == 77).all() for a in arr.values()), change
    st, arr, _keep = raw_call(gen, inp, outs=("verdict", "t_free"))        # no status
    assert st == abi.DIRECT_ERR_INVALID and (arr["verdict"] == 77).all()
    lib = cluster._lib()
    st, arr, (par, *_keep) = raw_call(gen, inp)
    assert st == abi.DIRECT_OK and (arr["status"] == 0).all()
    o = cluster.PlanCheckOut(status=arr["status"].ctypes.data)
    assert lib.direct_cluster_plan_check_batch(None, C.addressof(par), C.addressof(o)) == abi.DIRECT_ERR_INVALID
    assert lib.direct_cluster_plan_check_batch(gen.h, None, C.addressof(o)) == abi.DIRECT_ERR_INVALID
    assert lib.direct_cluster_plan_check_batch(gen.h, C.addressof(par), None) == abi.DIRECT_ERR_INVALID
    bare = cluster.ClusterGenerator(mh.DIMS, max_batch=2, cluster_capacity=64, candidate_capacity=64)   # a handle without a map
    arr["status"][:] = 77
    assert lib.direct_cluster_plan_check_batch(bare.h, C.addressof(par), C.addressof(o)) == abi.DIRECT_ERR_INVALID
    assert (arr["status"] == 77).all() and b"map" in lib.direct_cluster_last_error()
    bare.close()


def test_refusals_name_their_cause(gen, inputs):
    """every single fault is refused in its own words, and of two faults the one the call tests first is named"""
    inp = ph.pick(inputs["random7"], "bez")
    last = cluster._lib().direct_cluster_last_error
    for change, words in FAULTS:
        st, _arr, _keep = raw_call(gen, inp, **change)
        assert st == abi.DIRECT_ERR_INVALID and words in last(), (change, last())
    pairs = [(dict(depth=13, resolution=0.0), b"depth outside"), (dict(outside_blocks=2, resolution=0.0), b"outside_blocks"),
             (dict(resolution=0.0, margin=-1.0), b"resolution must be"), (dict(margin=-1.0, map_lower=NAN3), b"margin must be"),
             (dict(mem=2, dtype=2), b"neither DIRECT_MEM_HOST")]
    for change, words in pairs:
        st, _arr, _keep = raw_call(gen, inp, **change)
        assert st == abi.DIRECT_ERR_INVALID and words in last(), (change, last())
    bare = cluster.ClusterGenerator(mh.DIMS, max_batch=2, cluster_capacity=64, candidate_capacity=64)   # a handle without a map
    st, _arr, _keep = raw_call(bare, inp, depth=13)
    assert st == abi.DIRECT_ERR_INVALID and b"depth outside" in last(), last()
    st, _arr, _keep = raw_call(bare, inp)
    assert st == abi.DIRECT_ERR_INVALID and b"the handle has no map" in last(), last()
    bare.close()


def test_optional_outputs_may_be_null(gen, grid, inputs):
    inp = ph.pick(inputs["crafted"], "bez")
    want = ph.restate(inp, grid, 5, use_t_from=False)
    st, arr, _keep = raw_call(gen, inp, outs=("status",))
    assert st == abi.DIRECT_OK and np.array_equal(arr["status"], want["status"]) and (arr["verdict"] == 77).all()
    st, arr, _keep = raw_call(gen, inp, outs=("status", "t_free", "hit_box"))
    assert st == abi.DIRECT_OK and np.array_equal(arr["t_free"], want["t_free"]) and np.array_equal(arr["hit_box"], want["hit_box"])
    assert (arr["seg_first"] == 77).all() and gen.last_ms() > 0.0


def test_resident_clusters_and_paths_stay(gen, grid, inputs):
    """a check between a generation and its hull, and between two path queries, changes neither"""
    free = np.argwhere(grid[:20] == 0)
    seeds = free[np.random.default_rng(7).choice(len(free), 4, replace=False)].astype(np.int32)
    inp = ph.pick(inputs["long5"], "poly")

    def hull(with_check):
        gen.polygon_generation(seeds, fetch_clusters=False)
        if with_check:
            check(gen, inp, 7)
        return gen.hull_planes(ph.RES, ph.LOWER, batch=4)
    a, b = hull(False), hull(True)
    assert np.array_equal(a["rtn"], b["rtn"]) and np.array_equal(a["n_planes"], b["n_planes"])
    assert all(np.array_equal(x, y) for x, y in zip(a["plane_int"], b["plane_int"]))
    p0 = gen.grid_paths(seeds[:2], seeds[2:])
    check(gen, inp, 7)
    p1 = gen.grid_paths(seeds[:2], seeds[2:])
    assert np.array_equal(p0["rtn"], p1["rtn"]) and np.array_equal(p0["path_len"], p1["path_len"])
    assert all(np.array_equal(x, y) for x, y in zip(p0["paths"], p1["paths"]))
    assert np.array_equal(p0["path_cost"].view(np.int64), p1["path_cost"].view(np.int64))
