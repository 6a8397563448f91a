"""direct_cluster_plan_clearance_batch on the GPU against the NumPy restatement of tests/dist_field_harness.py, which evaluates
every leaf: equal outputs, integer for integer and bit for bit of every double.  No tolerance anywhere: HIP's double sqrt is correctly
rounded without fast-math and the build passes no such flag; a last-bit difference would be a finding to report with its input."""
import ctypes as C

import numpy as np
import pytest

from direct_amd import abi, cluster
from tests import dist_field_harness as dh
from tests import map_cloud_harness as mh
from tests import plan_check_harness as ph

pytestmark = pytest.mark.gpu
OUTS = dh.KEYS


@pytest.fixture(scope="module")
def grid():
    return ph.shared_map()


@pytest.fixture(scope="module")
def field(grid):
    return dh.brute_d2(grid)


@pytest.fixture(scope="module")
def gen(built, grid, field):
    g = cluster.ClusterGenerator(mh.DIMS, max_batch=4, cluster_capacity=2048, candidate_capacity=512)
    g.set_map(grid)
    g.build_distance_field()
    assert np.array_equal(g.distance_field(), field)
    yield g
    g.close()


@pytest.fixture(scope="module")
def inputs():
    return dh.clear_inputs()


def clearance(gen, inp, depth, radius=0.0, use_t_from=True, device=False):
    """plan_clearance on an input dict of the harness (one of bez / poly), from host arrays or from device tensors -> NumPy outputs"""
    kind = "poly" if inp.get("poly") is not None else "bez"
    args = dict(n_seg=inp["n_seg"], T=inp["T"], t_from=inp.get("t_from") if use_t_from else None)
    args[kind] = inp[kind]
    if device:
        import torch
        args = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")) for k, v in args.items()}
    out = gen.plan_clearance(map_lower=ph.LOWER, resolution=ph.RES, depth=depth, radius=radius, **args)
    return {k: (v.cpu().numpy() if device else v) for k, v in out.items()}


@pytest.mark.parametrize("depth", [0, 1, 5, 6, 7, 12])
def test_outputs_equal_the_restatement(gen, field, inputs, depth):
    names = ("random7", "crafted", "invalid9", "leaving1") + (("long5",) if depth <= 7 else ())
    for name in names:
        for n, (kind, f32, use_t_from, radius) in enumerate(dh.COMBOS):
            inp = ph.pick(inputs[name], kind)
            inp = ph.as_f32(inp) if f32 else inp
            want = dh.restate_clearance(inp, field, depth, radius, use_t_from)
            for device in ((False, True) if n < 2 else (n == 3,)):
                got = clearance(gen, inp, depth, radius, use_t_from, device)
                dh.assert_same(got, want, f"{name} D={depth} {kind} f32={f32} device={device} t_from={use_t_from} radius={radius}")
    assert gen.last_ms() > 0.0


def test_a_capped_field(built, grid, field, inputs):
    g = cluster.ClusterGenerator(mh.DIMS, max_batch=4, cluster_capacity=64, candidate_capacity=64)
    g.set_map(grid)
    g.build_distance_field(4)
    inp = ph.pick(inputs["random7"], "bez")
    want = dh.restate_clearance(inp, np.minimum(field, 16).astype(np.int32), 6, 0.3)
    dh.assert_same(clearance(g, inp, 6, 0.3), want, "cap 4")
    g.set_map(np.zeros(mh.DIMS, np.uint8))                # an empty map: nothing to be near to
    g.build_distance_field()
    out = clearance(g, inp, 6, 0.3)
    assert np.isinf(out["clearance"]).all() and (out["verdict"] == 0).all() and (out["where"] == -1).all()
    g.close()


def rows_of(inp, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in inp.items()}


@pytest.mark.parametrize("name", ["crafted", "long5"])
def test_launch_shape(gen, inputs, name):
    """every row alone, two calls of halves and a permuted batch give the rows of the one call"""
    inp = ph.pick(inputs[name], "poly")
    B = len(inp["n_seg"])
    whole = clearance(gen, inp, 7, 0.3)
    h = B // 2
    halves = [clearance(gen, rows_of(inp, slice(0, h)), 7, 0.3), clearance(gen, rows_of(inp, slice(h, B)), 7, 0.3)]
    perm = np.random.default_rng(5).permutation(B)
    shuffled = clearance(gen, rows_of(inp, perm), 7, 0.3)
    for k in OUTS:
        assert np.array_equal(np.concatenate([halves[0][k], halves[1][k]]), whole[k], equal_nan=True), k
        assert np.array_equal(shuffled[k], whole[k][perm], equal_nan=True), k
    for b in range(B):
        one = clearance(gen, rows_of(inp, slice(b, b + 1)), 7, 0.3)
        for k in OUTS:
            assert np.array_equal(one[k][0], whole[k][b], equal_nan=True), (k, b)


def raw_call(g, inp, outs=OUTS, **change):
    """the C call on host arrays with fields of the input struct replaced -> (status code, output arrays prefilled with 77)"""
    kind = "poly" if inp.get("poly") is not None else "bez"
    T, coef, n_seg = (np.ascontiguousarray(inp["T"], np.float64), np.ascontiguousarray(inp[kind], np.float64),
                      np.ascontiguousarray(inp["n_seg"], np.int32))
    B, N = T.shape
    par = cluster.PlanClearIn(batch=B, n_seg_max=N, mem=abi.MEM_HOST, dtype=abi.F64, n_seg=n_seg.ctypes.data, T=T.ctypes.data,
                              map_lower=(C.c_double * 3)(*ph.LOWER), resolution=ph.RES, radius=0.3, depth=5)
    setattr(par, kind, coef.ctypes.data)
    for k, v in change.items():
        setattr(par, k, v)
    arr = dict(status=np.full(B, 77, np.int32), verdict=np.full(B, 77, np.int32), where=np.full((B, 2), 77, np.int32), clearance=np.full(B, 77.0),
               t_min=np.full(B, 77.0), t_free=np.full(B, 77.0), seg_clearance=np.full((B, N), 77.0))
    o = cluster.PlanClearOut(**{k: arr[k].ctypes.data for k in outs})
    return cluster._lib().direct_cluster_plan_clearance_batch(g.h, C.addressof(par), C.addressof(o)), arr, (par, T, coef, n_seg)


NAN3, SOME = (C.c_double * 3)(0.0, float("nan"), 0.0), np.zeros(8)
# every single fault with the words of its refusal, as direct_cluster_last_error() gives them
FAULTS = [(dict(n_seg=None), b"null argument"), (dict(T=None), b"null argument"), (dict(batch=0), b"batch and n_seg_max must be positive"),
          (dict(batch=-1), b"batch and n_seg_max must be positive"), (dict(n_seg_max=0), b"batch and n_seg_max must be positive"),
          (dict(bez=None), b"exactly one of bez and poly"), (dict(poly=SOME.ctypes.data), b"exactly one of bez and poly"),
          (dict(mem=2), b"neither DIRECT_MEM_HOST"), (dict(dtype=2), b"dtype is neither"), (dict(depth=-1), b"depth outside"),
          (dict(depth=13), b"depth outside"), (dict(map_lower=NAN3), b"map_lower"), (dict(radius=-0.1), b"radius must be"),
          (dict(radius=float("nan")), b"radius must be"), (dict(radius=float("inf")), b"radius must be"), (dict(resolution=0.0), b"resolution must be"),
          (dict(resolution=-1.0), b"resolution must be"), (dict(resolution=float("inf")), b"resolution must be"),
          (dict(resolution=float("nan")), b"resolution must be")]


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
    o = cluster.PlanClearOut(status=arr["status"].ctypes.data)
    assert lib.direct_cluster_plan_clearance_batch(None, C.addressof(par), C.addressof(o)) == abi.DIRECT_ERR_INVALID
    assert lib.direct_cluster_plan_clearance_batch(gen.h, None, C.addressof(o)) == abi.DIRECT_ERR_INVALID
    assert lib.direct_cluster_plan_clearance_batch(gen.h, C.addressof(par), None) == abi.DIRECT_ERR_INVALID
    bare = cluster.ClusterGenerator(mh.DIMS, max_batch=2, cluster_capacity=64, candidate_capacity=64)   # a handle without a map
    arr["status"][:] = 77
    assert lib.direct_cluster_plan_clearance_batch(bare.h, C.addressof(par), C.addressof(o)) == abi.DIRECT_ERR_INVALID
    assert (arr["status"] == 77).all() and b"map" in lib.direct_cluster_last_error()
    bare.set_map(np.zeros(mh.DIMS, np.uint8))                              # a map, but no field
    assert lib.direct_cluster_plan_clearance_batch(bare.h, C.addressof(par), C.addressof(o)) == abi.DIRECT_ERR_INVALID
    assert (arr["status"] == 77).all() and b"distance field" in lib.direct_cluster_last_error()
    bare.close()


def test_refusals_name_their_cause(gen, inputs):
    """every single fault is refused in its own words, and of two faults the one the call tests first is named"""
    inp = ph.pick(inputs["random7"], "bez")
    last = cluster._lib().direct_cluster_last_error
    for change, words in FAULTS:
        st, _arr, _keep = raw_call(gen, inp, **change)
        assert st == abi.DIRECT_ERR_INVALID and words in last(), (change, last())
    pairs = [(dict(depth=13, resolution=0.0), b"depth outside"), (dict(resolution=0.0, radius=-1.0), b"resolution must be"),
             (dict(radius=-1.0, map_lower=NAN3), b"radius must be"), (dict(mem=2, dtype=2), b"neither DIRECT_MEM_HOST")]
    for change, words in pairs:
        st, _arr, _keep = raw_call(gen, inp, **change)
        assert st == abi.DIRECT_ERR_INVALID and words in last(), (change, last())
    bare = cluster.ClusterGenerator(mh.DIMS, max_batch=2, cluster_capacity=64, candidate_capacity=64)   # a handle without a map
    st, _arr, _keep = raw_call(bare, inp, depth=13)
    assert st == abi.DIRECT_ERR_INVALID and b"depth outside" in last(), last()
    st, _arr, _keep = raw_call(bare, inp)
    assert st == abi.DIRECT_ERR_INVALID and b"the handle has no map" in last(), last()
    bare.set_map(np.zeros(mh.DIMS, np.uint8))                              # a map, but no field: named before the slot count
    st, arr, _keep = raw_call(bare, inp, batch=1 << 16, n_seg_max=1 << 15)
    assert st == abi.DIRECT_ERR_INVALID and b"no valid distance field" in last(), last()
    assert all((a == 77).all() for a in arr.values())
    bare.close()


def test_calls_alternate_on_one_handle(gen, grid, field, inputs):
    """check_plans of 7 x 5, plan_clearance of a 3 x 2 slice, check_plans again: each call reads its own workspace and its own rows"""
    inp = ph.pick(inputs["random7"], "poly")
    part = dict(n_seg=np.minimum(inp["n_seg"][:3], 2), T=np.ascontiguousarray(inp["T"][:3, :2]), poly=np.ascontiguousarray(inp["poly"][:3, :2]),
                t_from=inp["t_from"][:3])
    want = ph.restate(inp, grid, 7, 0.2)

    def check():
        return gen.check_plans(inp["n_seg"], inp["T"], ph.LOWER, ph.RES, poly=inp["poly"], depth=7, margin=0.2, t_from=inp["t_from"])
    ph.assert_same(check(), want, "check before")
    dh.assert_same(clearance(gen, part, 7, 0.3), dh.restate_clearance(part, field, 7, 0.3), "clearance between")
    ph.assert_same(check(), want, "check after")


def test_optional_outputs_may_be_null(gen, field, inputs):
    inp = ph.pick(inputs["crafted"], "bez")
    want = dh.restate_clearance(inp, field, 5, 0.3, use_t_from=False)
    st, arr, _keep = raw_call(gen, inp, outs=("status",))
    assert st == abi.DIRECT_OK and np.array_equal(arr["status"], want["status"]) and (arr["clearance"] == 77).all()
    st, arr, _keep = raw_call(gen, inp, outs=("status", "clearance", "where"))
    assert st == abi.DIRECT_OK and np.array_equal(arr["clearance"], want["clearance"]) and np.array_equal(arr["where"], want["where"])
    assert (arr["seg_clearance"] == 77).all() and (arr["t_free"] == 77).all() and gen.last_ms() > 0.0
