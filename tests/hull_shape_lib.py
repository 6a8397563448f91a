"""Shapes for the hull -> planes tests beyond grown blobs (tests/test_hull.py on the host build of hull_core.h,
tests/test_gpu_hull.py on the device, tests/golden/make_hull_golden.py for the committed oracle results), and the
comparison both suites use.  Plain NumPy; every builder is deterministic, so the clusters themselves are not committed.

Each shape has the smallest size that still reaches its path:
  ext_*     clusters that span most of a 1023 x 1023 x 64 map.  hull::edge_test's tie-break Ru u + Rv v is a product of
            two projections v = w . (d x e1) ~ |w| |d|^2: for the eight corners of a box with x / y extent E voxels the box
            edge along x meets the corners of the opposite face with v = +/- 8 E^3 (lattice units, twice the voxel index),
            and v^2 = 64 E^6 reaches 2^63 between E = 724 (9.2175e18) and E = 725 (9.2942e18).  ext_box724 / ext_box725
            are that pair; ext_13 and ext_box{255,511,767,1022} carry five more voxels inside the box and on its faces.
  ball_*    voxel shells (R - 1.8)^2 < d^2 <= R^2: hundreds of candidates, planes and corners; R = 30.5 has more than
            hull::kCandCap (2048) line-extreme points
  disc_*    discs in one layer (flat: the eight corners of every voxel, > 256 lattice points, corners duplicated across
            the 256-point chunks of the compactions), flat in z, x and y; disc_plus is one voxel away from flat
  sheet     the diagonal sheet that is not full-dimensional (code 3)
  box_cap   a solid 32 x 32 x 20 box: exactly as many voxels as the device tests' cluster capacity
"""
import numpy as np

RES, LOWER = 0.2, np.array([-12.0, -12.0, 0.0])
KEYS = ("plane_int", "planes", "vertices", "center")
BIG_MAP, SMALL_MAP = (1023, 1023, 64), (96, 96, 96)
OVERFLOW_AT = 725      # smallest x / y extent of a box-corner set whose tie-break product leaves 64 bits (see above)


def box_corners(ex, ez=63, extras=True):
    """the eight corners of [0, ex] x [0, ex] x [0, ez] and, with `extras`, five voxels inside it and on its faces"""
    pts = [[x, y, z] for z in (0, ez) for y in (0, ex) for x in (0, ex)]
    if extras:
        pts += [[ex // 2, 3, 1], [3, (ex * 7) // 10, ez - 1], [ex - 22, ex - 21, ez // 2], [17, ex, 5], [ex, 19, (ez * 7) // 10]]
    return np.array(pts, np.int32)


def thirteen():
    return np.array([[0, 0, 0], [1022, 0, 0], [0, 1022, 0], [1022, 1022, 0], [0, 0, 63], [1022, 0, 63], [0, 1022, 63],
                     [1022, 1022, 63], [511, 3, 1], [3, 700, 62], [1000, 1001, 31], [17, 1022, 5], [1022, 19, 44]], np.int32)


def ball_shell(R):
    c = int(np.ceil(R)) + 1
    g = np.arange(2 * c + 1) - c
    d2 = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
    return np.argwhere((d2 > (R - 1.8) ** 2) & (d2 <= R * R)).astype(np.int32)


def disc(R, axis=2, layer=5):
    """voxels within R of the centre of one layer; axis: the coordinate they share"""
    c = int(np.ceil(R)) + 1
    g = np.arange(2 * c + 1) - c
    uv = np.argwhere(g[:, None] ** 2 + g[None, :] ** 2 <= R * R)
    return np.insert(uv, axis, layer, axis=1).astype(np.int32)


def disc_plus():
    return np.concatenate([disc(10.5), [[12, 12, 6]]]).astype(np.int32)


def sheet():
    return np.array([[x, x, z] for x in range(5) for z in range(4)], np.int32)


def box_cap():
    return np.array([[x, y, z] for x in range(2, 34) for y in range(3, 35) for z in range(1, 21)], np.int32)


# name -> (builder, map the device tests put it on, the oracle answers within a second)
SHAPES = {"ext_13": (thirteen, BIG_MAP, True)}
for _e in (255, 511, 767, 1022):
    SHAPES["ext_box%d" % _e] = (lambda e=_e: box_corners(e), BIG_MAP, True)
for _e in (OVERFLOW_AT - 1, OVERFLOW_AT):
    SHAPES["ext_box%d" % _e] = (lambda e=_e: box_corners(e, extras=False), BIG_MAP, True)
SHAPES["ball_6.5"] = (lambda: ball_shell(6.5), SMALL_MAP, True)
SHAPES["ball_10.5"] = (lambda: ball_shell(10.5), SMALL_MAP, False)
SHAPES["ball_15.5"] = (lambda: ball_shell(15.5), SMALL_MAP, False)
for _r in (10.5, 25.5, 40.5):
    for _a in (2, 0, 1):
        SHAPES["disc_%s_%s" % (_r, "xyz"[_a])] = (lambda r=_r, a=_a: disc(r, a), SMALL_MAP, True)
SHAPES["disc_plus"] = (disc_plus, SMALL_MAP, True)
SHAPES["sheet"] = (sheet, SMALL_MAP, True)
SHAPES["box_cap"] = (box_cap, SMALL_MAP, True)
# more line-extreme points than hull::kCandCap: no oracle run (brute force over triples of thousands of points); the expected answer is the refusal
OVERFLOW_SHAPE = "ball_30.5"
EXTENT = [n for n in SHAPES if n.startswith("ext_")]
PLANE_CAP, VERT_CAP = 512, 1024   # capacities of every fixture row and of the tests that compare with it


def build(name):
    return ball_shell(30.5) if name == OVERFLOW_SHAPE else SHAPES[name][0]()


def fixture_row(fix, name):
    """the oracle's answer for `name` out of tests/golden/hull_shapes.npz, as oracle.hullapi.hull_planes returns it"""
    if name == OVERFLOW_SHAPE:
        z = np.zeros
        return dict(rc=1, degenerate=0, n_planes=0, n_vertices=0, plane_int=z((0, 4), np.int64), planes=z((0, 4)),
                    vert_q=z((0, 3), np.int32), vertices=z((0, 3)), center=None)
    r = {k: fix["%s/%s" % (name, k)] for k in ("plane_int", "planes", "vert_q", "vertices", "center")}
    r.update(rc=int(fix["%s/rc" % name]), degenerate=int(fix["%s/degenerate" % name]))
    r.update(n_planes=len(r["plane_int"]), n_vertices=len(r["vert_q"]))
    return r


def assert_same(got, ref, what=""):
    """`got` (host build, oracle or one device row as a dict) equals the oracle's `ref` bit for bit"""
    for k in ("rc", "degenerate", "n_planes", "n_vertices"):
        assert int(got[k]) == int(ref[k]), (what, k, int(got[k]), int(ref[k]))
    if ref["rc"] != 0:
        return
    for k in KEYS + (("vert_q",) if "vert_q" in got else ()):
        assert np.array_equal(got[k], ref[k]), (what, k)


def device_row(dev, b):
    """row b of ClusterGenerator.hull_planes as the dict assert_same compares"""
    return dict(rc=dev["rtn"][b], degenerate=dev["degenerate"][b], n_planes=dev["n_planes"][b], n_vertices=dev["n_vertices"][b],
                plane_int=dev["plane_int"][b], planes=dev["planes"][b], vertices=dev["vertices"][b], center=dev["center"][b])
