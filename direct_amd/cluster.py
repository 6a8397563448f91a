"""Python binding of the corridor-cluster generator of libdirect_ddp.so (include/direct_cluster.h) for tests and
tools.  Mirrors cudaPolytopeGeneration's calling protocol (polyhedron_generator/include/polyhedron_generator/
cluster_server_cpu.h:54-74): paramSet -> ClusterGenerator(...), setObs/mapUpload -> set_map, polygonGeneration ->
polygon_generation (for a batch of seed voxels).  No CPU fallback."""
import ctypes as C

import numpy as np

from . import abi, solver


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32), ("max_z", C.c_int32),
                ("max_batch", C.c_int32), ("cluster_capacity", C.c_int32), ("candidate_capacity", C.c_int32),
                ("reserved", C.c_int32)]


class MapCloud(C.Structure):  # direct_map_cloud_t
    _fields_ = [("map_lower", C.c_double * 3), ("map_upper", C.c_double * 3), ("resolution", C.c_double),
                ("cloud_margin", C.c_double), ("border", C.c_int32), ("mode", C.c_int32), ("stride", C.c_int32),
                ("reserved", C.c_int32)]


class MapScan(C.Structure):  # direct_map_scan_t
    _fields_ = [("map_lower", C.c_double * 3), ("map_upper", C.c_double * 3), ("resolution", C.c_double), ("max_range", C.c_double),
                ("origin", C.c_double * 3), ("inflate", C.c_int32 * 3), ("mode", C.c_int32), ("stride", C.c_int32),
                ("flags", C.c_int32)]


class MapEvidence(C.Structure):  # direct_map_evidence_t
    _fields_ = [("scan", MapScan), ("hit", C.c_int32), ("miss", C.c_int32), ("ev_min", C.c_int32), ("ev_max", C.c_int32),
                ("occ", C.c_int32), ("reserved", C.c_int32 * 3)]


class FrontierIn(C.Structure):  # direct_frontier_in_t
    _fields_ = [("min_d2", C.c_int32), ("min_size", C.c_int32), ("capacity", C.c_int32), ("mem", C.c_int32)]


class FrontierOut(C.Structure):  # direct_frontier_out_t
    _fields_ = [("label", C.c_void_p), ("size", C.c_void_p), ("centroid", C.c_void_p), ("rep", C.c_void_p), ("voxel_label", C.c_void_p),
                ("stats", C.c_void_p)]


class ViewGainIn(C.Structure):  # direct_view_gain_in_t
    _fields_ = [("range_vox", C.c_double), ("n", C.c_int32), ("n_dirs", C.c_int32), ("n_sets", C.c_int32), ("mem_in", C.c_int32),
                ("mem", C.c_int32)]


class ViewGainIO(C.Structure):  # direct_view_gain_io_t
    _fields_ = [("voxel", C.c_void_p), ("set", C.c_void_p), ("dirs", C.c_void_p), ("code", C.c_void_p), ("gain", C.c_void_p),
                ("seen", C.c_void_p), ("ends", C.c_void_p)]


class PlanCheckIn(C.Structure):  # direct_plan_check_in_t
    _fields_ = [("batch", C.c_int32), ("n_seg_max", C.c_int32), ("mem", C.c_int32), ("dtype", C.c_int32), ("n_seg", C.c_void_p),
                ("T", C.c_void_p), ("bez", C.c_void_p), ("poly", C.c_void_p), ("map_lower", C.c_double * 3), ("resolution", C.c_double),
                ("margin", C.c_double), ("depth", C.c_int32), ("outside_blocks", C.c_int32), ("t_from", C.c_void_p)]


class PlanCheckOut(C.Structure):  # direct_plan_check_out_t
    _fields_ = [("status", C.c_void_p), ("verdict", C.c_void_p), ("t_free", C.c_void_p), ("first", C.c_void_p),
                ("hit_box", C.c_void_p), ("seg_first", C.c_void_p), ("stats", C.c_void_p)]


PlanClearIn, PlanClearOut = abi.PlanClearIn, abi.PlanClearOut  # direct_plan_clear_in_t, direct_plan_clear_out_t
CubeCorridorIn, CubeCorridorOut = abi.CubeCorridorIn, abi.CubeCorridorOut  # direct_cube_corridor_in_t, direct_cube_corridor_out_t
GridPathClearIn, GridPathClearOut = abi.GridPathClearIn, abi.GridPathClearOut  # direct_grid_path_clear_in_t, direct_grid_path_clear_out_t
GridPathFanIn, GridPathFanOut = abi.GridPathFanIn, abi.GridPathFanOut  # direct_grid_path_fan_in_t, direct_grid_path_fan_out_t
ReachableIn, ReachableOut = abi.ReachableIn, abi.ReachableOut  # direct_reachable_in_t, direct_reachable_out_t
ClusterCorridorIn, ClusterCorridorOut = abi.ClusterCorridorIn, abi.ClusterCorridorOut  # direct_cluster_corridor_in_t, direct_cluster_corridor_out_t


EXPORTS = ("direct_cluster_create", "direct_cluster_destroy", "direct_cluster_last_error", "direct_cluster_set_map",
           "direct_cluster_polygon_generation_batch", "direct_cluster_convex_test", "direct_cluster_last_ms",
           "direct_cluster_set_stream", "direct_cluster_hull_planes_batch", "direct_cluster_grid_path_batch",
           "direct_cluster_map_from_cloud", "direct_cluster_get_map", "direct_cluster_plan_check_batch",
           "direct_cluster_distance_field", "direct_cluster_get_distance_field", "direct_cluster_plan_clearance_batch",
           "direct_cluster_cube_corridor_batch", "direct_cluster_grid_path_clear_batch", "direct_cluster_grid_path_fan_batch",
           "direct_cluster_cube_corridor_clear_batch", "direct_cluster_free_components", "direct_cluster_get_free_components",
           "direct_cluster_reachable_batch", "direct_cluster_corridor_batch", "direct_cluster_map_integrate_scan",
           "direct_cluster_get_scan_grid", "direct_cluster_scan_phase_ms", "direct_cluster_get_known", "direct_cluster_set_known",
           "direct_cluster_frontier", "direct_cluster_frontier_phase_ms", "direct_cluster_view_gain_batch",
           "direct_cluster_map_integrate_scan_evidence", "direct_cluster_get_evidence", "direct_cluster_set_evidence",
           "direct_cluster_evidence_phase_ms", "direct_cluster_set_unknown_policy", "direct_cluster_get_unknown_policy",
           "direct_cluster_get_open_map")
CLUSTER_OK, CLUSTER_OVERFLOW, CLUSTER_BAD_SEED = 0, 1, 2
HULL_OK, HULL_OVERFLOW, HULL_BAD_VOXEL, HULL_FLAT = 0, 1, 2, 3
GRID_PATH_OK, GRID_PATH_NO_PATH, GRID_PATH_BAD_ENDPOINT, GRID_PATH_OVERFLOW, GRID_PATH_ROUND_LIMIT = 0, 1, 2, 3, 4
MAP_BORDER_CLAMP, MAP_BORDER_DROP = 0, 1
MAP_REPLACE, MAP_ADD = 0, 1
SCAN_RESET, SCAN_CONTINUE, SCAN_ADOPT = 0, 1, 2
SCAN_TRACK_KNOWN = 1   # direct_map_scan_t.flags
UNKNOWN_FREE, UNKNOWN_OCCUPIED = 0, 1
UNKNOWN_POLICIES = ("free", "occupied")   # by value
VIEW_OK, VIEW_OUTSIDE, VIEW_OCCUPIED, VIEW_BAD_SET = 0, 1, 2, 3
VIEW_ENDS = ("blocked", "left", "range", "skipped")   # ends[c][4]
FRONTIER_STATS = ("known", "frontier", "components", "kept", "written", "largest")   # stats[6]
SCAN_STATS = ("points", "skipped_nonfinite", "truncated", "outside", "raw_occupied", "occupied", "set", "cleared")   # stats[8]
EVIDENCE_STATS = SCAN_STATS + ("touched_hit", "touched_pass", "positive", "negative")   # stats[12]
PLAN_CHECK_INVALID = -1
DIST_NONE = 0x7fffffff
CUBE_CORRIDOR_OK, CUBE_CORRIDOR_OVERFLOW, CUBE_CORRIDOR_BAD_PATH = 0, 1, 2
CLUSTER_CORRIDOR_OK, CLUSTER_CORRIDOR_OVERFLOW, CLUSTER_CORRIDOR_BAD_PATH = 0, 1, 2
CLUSTER_CORRIDOR_NO_POLYTOPE, CLUSTER_CORRIDOR_TOO_MANY_PLANES = 3, 4
_BOUND = False


def _lib():
    global _BOUND
    L = solver.lib()
    if not _BOUND:
        L.direct_cluster_last_error.restype = C.c_char_p
        L.direct_cluster_create.argtypes = [C.c_void_p, C.c_void_p]
        L.direct_cluster_destroy.argtypes = [C.c_void_p]
        L.direct_cluster_set_map.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_polygon_generation_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                               C.c_int32] + [C.c_void_p] * 5
        L.direct_cluster_convex_test.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_last_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.direct_cluster_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.direct_cluster_hull_planes_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                                        C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 8
        L.direct_cluster_grid_path_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                      C.c_int32] + [C.c_void_p] * 6
        L.direct_cluster_map_from_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.direct_cluster_get_map.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_plan_check_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_distance_field.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_get_distance_field.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_plan_clearance_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_cube_corridor_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_grid_path_clear_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_grid_path_fan_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_cube_corridor_clear_batch.argtypes = list(abi.CUBE_CORRIDOR_CLEAR_ARGTYPES)
        L.direct_cluster_free_components.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_get_free_components.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_reachable_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_corridor_batch.argtypes = list(abi.CLUSTER_CORRIDOR_ARGTYPES)
        L.direct_cluster_map_integrate_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.direct_cluster_get_scan_grid.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_scan_phase_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.direct_cluster_get_known.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_set_known.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_frontier.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_frontier_phase_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.direct_cluster_view_gain_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_map_integrate_scan_evidence.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.direct_cluster_get_evidence.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_set_evidence.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.direct_cluster_evidence_phase_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.direct_cluster_set_unknown_policy.argtypes = [C.c_void_p, C.c_int32]
        L.direct_cluster_get_unknown_policy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.direct_cluster_get_open_map.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        _BOUND = True
    return L


def clearance_penalty_table(weight, soft_radius_vox):
    """A penalty table for grid_paths_clear, indexed by the stored D2: weight * (1 - sqrt(d2) / soft_radius_vox)^2 for every
    d2 < soft_radius_vox^2 (the entry at 0 is included; it is never read for a free voxel).  Pure NumPy, float64; beyond the table
    the penalty is 0."""
    r = float(soft_radius_vox)
    n = int(np.ceil(r * r)) if r > 0 else 0
    d2 = np.arange(n, dtype=np.float64)
    return float(weight) * (1.0 - np.sqrt(d2) / r) ** 2 if n else np.zeros(0, np.float64)


def view_directions(n_az, n_el, el_min, el_max, az_min=-np.pi, az_max=np.pi, yaw=0.0):
    """A direction set for view_gain: n_az x n_el unit vectors at the CENTRES of an even azimuth x elevation grid over
    [az_min, az_max] x [el_min, el_max] (radians; elevation from the horizontal plane, positive up), turned by `yaw` about z.
    Cell centres, so a full turn (the default azimuth span) has no doubled ray.  Built on the host with NumPy in float64 and
    rounded once -> float32 [n_az * n_el][3], azimuth major.  Stack several (np.stack) to make the sets of one call."""
    az = float(az_min) + (np.arange(int(n_az), dtype=np.float64) + 0.5) * ((float(az_max) - float(az_min)) / int(n_az)) + float(yaw)
    el = float(el_min) + (np.arange(int(n_el), dtype=np.float64) + 0.5) * ((float(el_max) - float(el_min)) / int(n_el))
    a, e = np.meshgrid(az, el, indexing="ij")
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1)
    return np.ascontiguousarray(d.reshape(-1, 3), np.float32)


def _check(st):
    if st != abi.DIRECT_OK:
        raise solver.DirectError(st, _lib().direct_cluster_last_error().decode())


class ClusterGenerator:
    def __init__(self, dims, max_batch=64, cluster_capacity=50000, candidate_capacity=10000, device=0):
        self.dims = tuple(int(d) for d in dims)
        self.device = int(device)
        self.max_batch, self.ccap, self.kcap = int(max_batch), int(cluster_capacity), int(candidate_capacity)
        cfg = Config(device, self.dims[0], self.dims[1], self.dims[2], self.max_batch, self.ccap, self.kcap, 0)
        h = C.c_void_p()
        _check(_lib().direct_cluster_create(C.addressof(cfg), C.addressof(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            _lib().direct_cluster_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_map(self, grid):
        g = np.ascontiguousarray(grid, np.uint8)
        assert g.shape == self.dims
        _check(_lib().direct_cluster_set_map(self.h, abi.MEM_HOST, g.ctypes.data))

    def set_map_from_cloud(self, points, map_lower, resolution, cloud_margin=0.25, map_upper=None, border="clamp", add=False):
        """The map from a point cloud, on the device (direct_cluster_map_from_cloud; stands where the reference runs
        rcvPointCloudCallBack, teach_repeat_planner.cpp:523-581).  points: a NumPy array or a device tensor of shape [n, 3] or
        [n, 4] (a pcl::PointXYZ buffer), float32.  border: "clamp" (the polytope generator's map) or "drop" (the path finder's;
        map_upper defaults to map_lower + dims * resolution).  add: keep the map the handle holds.
        -> dict(points, skipped_nonfinite, dropped, occupied)"""
        lower = np.asarray(map_lower, np.float64).reshape(3)
        upper = lower + np.asarray(self.dims, np.float64) * float(resolution) if map_upper is None else np.asarray(map_upper, np.float64).reshape(3)
        par = MapCloud((C.c_double * 3)(*lower), (C.c_double * 3)(*upper), float(resolution), float(cloud_margin),
                       {"clamp": MAP_BORDER_CLAMP, "drop": MAP_BORDER_DROP}[border], MAP_ADD if add else MAP_REPLACE, 0, 0)
        pts, mem, ptr = self._cloud(points)
        par.stride = int(pts.shape[1])
        n = int(pts.shape[0])
        stats = np.zeros(4, np.int64)
        _check(_lib().direct_cluster_map_from_cloud(self.h, C.addressof(par), n, mem, ptr if n else None, stats.ctypes.data))
        return dict(points=int(stats[0]), skipped_nonfinite=int(stats[1]), dropped=int(stats[2]), occupied=int(stats[3]))

    @staticmethod
    def _cloud(points):
        """-> (the array or tensor that owns the floats, mem, pointer) of a cloud given as NumPy or as a device tensor"""
        if isinstance(points, np.ndarray) or not hasattr(points, "data_ptr"):
            pts = np.ascontiguousarray(points, np.float32)
            pts = pts.reshape(0, 3) if pts.size == 0 and pts.ndim != 2 else pts
            mem, ptr = abi.MEM_HOST, pts.ctypes.data
        else:
            import torch
            pts = points.to(torch.float32).contiguous()
            assert pts.is_cuda
            torch.cuda.current_stream(pts.device).synchronize()  # the handle's stream is not torch's
            mem, ptr = abi.MEM_DEVICE, pts.data_ptr()
        assert pts.ndim == 2 and pts.shape[1] in (3, 4), "points must have shape [n, 3] or [n, 4]"
        return pts, mem, ptr

    def integrate_scan(self, points, origin, map_lower, resolution, max_range, inflate=(0, 0, 0), mode="continue", map_upper=None,
                       track_known=False):
        """One sensor scan folded into the resident map (direct_cluster_map_integrate_scan): every ray from origin to a point
        carves the scan grid free, every return within max_range marks its voxel, and the map is the scan grid dilated by the
        voxel box inflate.  points as in set_map_from_cloud.  mode: "reset" (the scan grid starts empty), "continue" (keep it) or
        "adopt" (it starts as the map the handle holds).  The field, the floor tables and the components stay valid when
        set + cleared == 0; rebuild them otherwise.  track_known: every voxel the scan carves or marks is also recorded in the
        resident known grid (known_grid, frontiers); an untracked scan drops a known grid the handle holds.
        -> dict(points, skipped_nonfinite, truncated, outside, raw_occupied, occupied, set, cleared)"""
        lower = np.asarray(map_lower, np.float64).reshape(3)
        upper = lower + np.asarray(self.dims, np.float64) * float(resolution) if map_upper is None else np.asarray(map_upper, np.float64).reshape(3)
        pts, mem, ptr = self._cloud(points)
        par = MapScan((C.c_double * 3)(*lower), (C.c_double * 3)(*upper), float(resolution), float(max_range),
                      (C.c_double * 3)(*np.asarray(origin, np.float64).reshape(3)), (C.c_int32 * 3)(*[int(v) for v in inflate]),
                      {"reset": SCAN_RESET, "continue": SCAN_CONTINUE, "adopt": SCAN_ADOPT}[mode], int(pts.shape[1]),
                      SCAN_TRACK_KNOWN if track_known else 0)
        n = int(pts.shape[0])
        stats = np.zeros(8, np.int64)
        _check(_lib().direct_cluster_map_integrate_scan(self.h, C.addressof(par), n, mem, ptr if n else None, stats.ctypes.data))
        return dict(zip(SCAN_STATS, (int(v) for v in stats)))

    def scan_grid(self):
        """The scan grid as a uint8 array of shape dims (direct_cluster_get_scan_grid): what the scans so far carved and marked,
        before the inflation"""
        g = np.zeros(self.dims, np.uint8)
        _check(_lib().direct_cluster_get_scan_grid(self.h, abi.MEM_HOST, g.ctypes.data))
        return g

    def known_grid(self):
        """The known grid as a uint8 array of shape dims (direct_cluster_get_known): 1 where a tracked scan has carved or marked
        (or set_known said so), 0 where nothing has been observed"""
        g = np.zeros(self.dims, np.uint8)
        _check(_lib().direct_cluster_get_known(self.h, abi.MEM_HOST, g.ctypes.data))
        return g

    def set_known(self, known):
        """The known grid becomes (known != 0) of a NumPy array or device tensor of shape dims, uint8; None: all zero
        (direct_cluster_set_known) - a persisted grid, a declared-known box around the take-off point, a prior map"""
        if known is None:
            mem, ptr = abi.MEM_HOST, None
        elif isinstance(known, np.ndarray) or not hasattr(known, "data_ptr"):
            known = np.ascontiguousarray(known, np.uint8)
            mem, ptr = abi.MEM_HOST, known.ctypes.data
        else:
            import torch
            known = known.to(torch.uint8).contiguous()
            assert known.is_cuda
            torch.cuda.current_stream(known.device).synchronize()  # the handle's stream is not torch's
            mem, ptr = abi.MEM_DEVICE, known.data_ptr()
        assert known is None or tuple(known.shape) == self.dims
        _check(_lib().direct_cluster_set_known(self.h, mem, ptr))

    def integrate_scan_evidence(self, points, origin, map_lower, resolution, max_range, hit=17, miss=8, ev_min=-40, ev_max=70, occ=1,
                                inflate=(0, 0, 0), mode="continue", map_upper=None, track_known=False):
        """One sensor scan folded into the resident EVIDENCE grid (direct_cluster_map_integrate_scan_evidence): every voxel a ray
        passes loses `miss`, every voxel a return lies in gains `hit` (a return beats a pass), once per voxel and scan, clamped to
        [ev_min, ev_max]; the scan grid is (evidence >= occ) and the map is the scan grid dilated by inflate.  The defaults are
        OctoMap's 0.85 / -0.4 / [-2, 3.5] / 0 log-odds in units of 0.05.  points, origin, inflate, map_upper and track_known as in
        integrate_scan.  mode: "reset" (the evidence starts at 0), "continue" (keep it) or "adopt" (ev_max where the map the handle
        holds is occupied, 0 elsewhere).  No points and "continue": re-threshold the evidence as it stands.
        -> dict of EVIDENCE_STATS: integrate_scan's eight, then touched_hit, touched_pass, positive, negative"""
        lower = np.asarray(map_lower, np.float64).reshape(3)
        upper = lower + np.asarray(self.dims, np.float64) * float(resolution) if map_upper is None else np.asarray(map_upper, np.float64).reshape(3)
        pts, mem, ptr = self._cloud(points)
        scan = MapScan((C.c_double * 3)(*lower), (C.c_double * 3)(*upper), float(resolution), float(max_range),
                       (C.c_double * 3)(*np.asarray(origin, np.float64).reshape(3)), (C.c_int32 * 3)(*[int(v) for v in inflate]),
                       {"reset": SCAN_RESET, "continue": SCAN_CONTINUE, "adopt": SCAN_ADOPT}[mode], int(pts.shape[1]),
                       SCAN_TRACK_KNOWN if track_known else 0)
        par = MapEvidence(scan, int(hit), int(miss), int(ev_min), int(ev_max), int(occ), (C.c_int32 * 3)(0, 0, 0))
        n = int(pts.shape[0])
        stats = np.zeros(12, np.int64)
        _check(_lib().direct_cluster_map_integrate_scan_evidence(self.h, C.addressof(par), n, mem, ptr if n else None, stats.ctypes.data))
        return dict(zip(EVIDENCE_STATS, (int(v) for v in stats)))

    def evidence_grid(self):
        """The evidence grid as an int8 array of shape dims (direct_cluster_get_evidence): what the evidence scans have counted per
        voxel, 0 where nothing is known"""
        g = np.zeros(self.dims, np.int8)
        _check(_lib().direct_cluster_get_evidence(self.h, abi.MEM_HOST, g.ctypes.data))
        return g

    def set_evidence(self, ev):
        """The evidence grid becomes a NumPy array or device tensor of shape dims, int8 (-128 is stored as -127); None: all zero
        (direct_cluster_set_evidence).  Map and scan grid follow at the next integrate_scan_evidence."""
        if ev is None:
            mem, ptr = abi.MEM_HOST, None
        elif isinstance(ev, np.ndarray) or not hasattr(ev, "data_ptr"):
            ev = np.ascontiguousarray(ev, np.int8)
            mem, ptr = abi.MEM_HOST, ev.ctypes.data
        else:
            import torch
            ev = ev.to(torch.int8).contiguous()
            assert ev.is_cuda
            torch.cuda.current_stream(ev.device).synchronize()  # the handle's stream is not torch's
            mem, ptr = abi.MEM_DEVICE, ev.data_ptr()
        assert ev is None or tuple(ev.shape) == self.dims
        _check(_lib().direct_cluster_set_evidence(self.h, mem, ptr))

    def evidence_phase_ms(self):
        """[touch, hit, fold, inflate, table] ms of the last evidence scan; the handle must have been created with
        DIRECT_CLUSTER_SCAN_TIMING=1"""
        ms = np.zeros(5, np.float32)
        _check(_lib().direct_cluster_evidence_phase_ms(self.h, ms.ctypes.data))
        return ms

    def set_unknown_policy(self, policy):
        """What the scans make of voxels nobody has observed (direct_cluster_set_unknown_policy): "free" (the default: their map
        byte is 0) or "occupied" (every scan keeps two grids: the open map, which is what it derives under "free", and the map,
        which is the open map with every unobserved voxel closed; every planning call reads the map, view_gain the open map).
        Takes effect at the next scan, which must be tracked under "occupied"; touches no grid."""
        _check(_lib().direct_cluster_set_unknown_policy(self.h, UNKNOWN_POLICIES.index(policy)))

    def unknown_policy(self):
        """-> dict(policy: "free" or "occupied", closed: voxels occupied in the map and free in the open map, open_ones: occupied
        voxels of the open map), the counts of the last successful scan under "occupied" (0 when the handle holds no open map)"""
        policy = C.c_int32(-1)
        stats = np.zeros(2, np.int64)
        _check(_lib().direct_cluster_get_unknown_policy(self.h, C.addressof(policy), stats.ctypes.data))
        return dict(policy=UNKNOWN_POLICIES[policy.value], closed=int(stats[0]), open_ones=int(stats[1]))

    def open_map(self):
        """The open map as a uint8 array of shape dims (direct_cluster_get_open_map): the map before unobserved space was closed;
        refused unless the last writer of the map was a successful "occupied" scan"""
        g = np.zeros(self.dims, np.uint8)
        _check(_lib().direct_cluster_get_open_map(self.h, abi.MEM_HOST, g.ctypes.data))
        return g

    def frontiers(self, min_size=1, min_d2=0, capacity=1024, mem="host", voxel_labels=False):
        """Goal voxels on the boundary between observed and unobserved space (direct_cluster_frontier): the 26-connected components
        of the known, enterable voxels (map byte 0 and, for min_d2 > 1, stored D2 >= min_d2) with an unknown face neighbour inside
        the map; those of at least min_size voxels, in ascending label order, the first `capacity` of them.
        -> dict(label [k], size [k], centroid [k][3], rep [k][3], stats: dict(known, frontier, components, kept, written, largest)
        and, with voxel_labels, voxel_label of shape dims), k = written.  rep is a member of its component: known, enterable and a
        legal goal of reachable / grid_paths_fan under the same floor.  mem="device": tensors (stats stays a dict)."""
        assert mem in ("host", "device")
        cap = int(capacity)
        if mem == "device":
            import torch
            z = lambda shape: torch.zeros(shape, dtype=torch.int32, device="cuda:%d" % self.device)
            ptr = lambda a: a.data_ptr()
        else:
            z = lambda shape: np.zeros(shape, np.int32)
            ptr = lambda a: a.ctypes.data
        out = dict(label=z(max(cap, 0)), size=z(max(cap, 0)), centroid=z((max(cap, 0), 3)), rep=z((max(cap, 0), 3)))
        vox = z(self.dims) if voxel_labels else None
        if mem == "device":
            torch.cuda.current_stream(out["label"].device).synchronize()  # the handle's stream is not torch's
        stats = np.zeros(6, np.int64)
        par = FrontierIn(int(min_d2), int(min_size), cap, abi.MEM_DEVICE if mem == "device" else abi.MEM_HOST)
        o = FrontierOut(*[ptr(out[k]) if cap > 0 else None for k in ("label", "size", "centroid", "rep")], None if vox is None else ptr(vox),
                        stats.ctypes.data)
        _check(_lib().direct_cluster_frontier(self.h, C.addressof(par), C.addressof(o)))
        k = int(stats[4])
        out = {key: a[:k] for key, a in out.items()}
        out["stats"] = dict(zip(FRONTIER_STATS, (int(v) for v in stats)))
        if voxel_labels:
            out["voxel_label"] = vox
        return out

    def view_gain(self, voxels, dirs, range_vox, sets=None, mem="host"):
        """How much unknown space an ideal sensor would see from each candidate voxel (direct_cluster_view_gain_batch): the rays
        of a direction set are walked from the centre of the voxel through the resident map, range_vox voxels far at most, until
        they hit an occupied voxel or leave the map.  voxels [n][3] int32 (frontiers()["rep"], say); dirs [n_dirs][3] or
        [n_sets][n_dirs][3] float32, map frame, any length (view_directions); sets [n] int32 or None (every candidate uses set 0):
        NumPy arrays or device tensors.  voxels decides the kind: beside device voxels (frontiers(mem="device")["rep"]) host dirs
        and sets are uploaded.  mem: where the outputs go ("host": NumPy, "device": tensors).
        -> dict(code [n] (VIEW_*), gain [n]: distinct visited voxels with known == 0, seen [n]: distinct visited voxels,
        ends [n][4]: rays that ended blocked, left the map, ran out of range, were skipped); a candidate whose code is not VIEW_OK
        has zeros."""
        assert mem in ("host", "device")
        if isinstance(voxels, np.ndarray) or not hasattr(voxels, "data_ptr"):
            vox = np.ascontiguousarray(voxels, np.int32).reshape(-1, 3)
            d = np.ascontiguousarray(dirs, np.float32)
            st = None if sets is None else np.ascontiguousarray(sets, np.int32).reshape(-1)
            mem_in, ptr_in = abi.MEM_HOST, lambda a: a.ctypes.data
        else:
            import torch
            vox = voxels.to(torch.int32).contiguous().reshape(-1, 3)
            up = lambda a: a if hasattr(a, "data_ptr") else torch.as_tensor(np.asarray(a), device=vox.device)  # host arrays follow the voxels
            d = up(dirs).to(torch.float32).contiguous()
            st = None if sets is None else up(sets).to(torch.int32).contiguous().reshape(-1)
            assert vox.is_cuda and d.is_cuda and (st is None or st.is_cuda)
            torch.cuda.current_stream(vox.device).synchronize()  # the handle's stream is not torch's
            mem_in, ptr_in = abi.MEM_DEVICE, lambda a: a.data_ptr()
        d = d.reshape((1,) + tuple(d.shape)) if d.ndim == 2 else d
        assert d.ndim == 3 and d.shape[2] == 3, "dirs must have shape [n_dirs, 3] or [n_sets, n_dirs, 3]"
        n = int(vox.shape[0])
        assert st is None or int(st.shape[0]) == n
        shapes = dict(code=(n,), gain=(n,), seen=(n,), ends=(n, 4))
        if mem == "host":
            out = {k: np.zeros(s, np.int32) for k, s in shapes.items()}
            ptr = lambda a: a.ctypes.data
        else:
            import torch
            out = {k: torch.zeros(s, dtype=torch.int32, device="cuda:%d" % self.device) for k, s in shapes.items()}
            torch.cuda.current_stream(out["code"].device).synchronize()  # the handle's stream is not torch's
            ptr = lambda a: a.data_ptr()
        par = ViewGainIn(float(range_vox), n, int(d.shape[1]), int(d.shape[0]), mem_in, abi.MEM_HOST if mem == "host" else abi.MEM_DEVICE)
        io = ViewGainIO(ptr_in(vox) if n else None, None if st is None or not n else ptr_in(st), ptr_in(d),
                        *[ptr(out[k]) if n else None for k in ("code", "gain", "seen", "ends")])
        _check(_lib().direct_cluster_view_gain_batch(self.h, C.addressof(par), C.addressof(io)))
        return out

    def frontier_phase_ms(self):
        """[mask, labelling, compaction, goals] ms of the last frontiers call; needs DIRECT_CLUSTER_SCAN_TIMING=1 at creation"""
        ms = (C.c_float * 4)()
        _check(_lib().direct_cluster_frontier_phase_ms(self.h, ms))
        return [float(v) for v in ms]

    def scan_phase_ms(self):
        """[carve, mark, inflate, table] ms of the last scan; the handle must have been created with DIRECT_CLUSTER_SCAN_TIMING=1"""
        ms = (C.c_float * 4)()
        _check(_lib().direct_cluster_scan_phase_ms(self.h, ms))
        return [float(v) for v in ms]

    def get_map(self):
        """The handle's map as a uint8 array of shape dims (direct_cluster_get_map)"""
        g = np.zeros(self.dims, np.uint8)
        _check(_lib().direct_cluster_get_map(self.h, abi.MEM_HOST, g.ctypes.data))
        return g

    def polygon_generation(self, seeds, itr_inflate_max=1000, itr_cluster_max=50, fetch_clusters=True):
        """-> dict(vertex_idx [B][24], clusters: list of [n][3] arrays, cluster_num, iters, rtn).  fetch_clusters=False:
        the voxels stay on the device (for hull_planes(batch=...)), clusters is None."""
        seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1, 3)
        B = seeds.shape[0]
        if not fetch_clusters:
            v = np.zeros((B, 24), np.int32)
            n, it, rtn = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
            _check(_lib().direct_cluster_polygon_generation_batch(self.h, B, seeds.ctypes.data, int(itr_inflate_max),
                                                                  int(itr_cluster_max), abi.MEM_HOST, v.ctypes.data, None,
                                                                  n.ctypes.data, it.ctypes.data, rtn.ctypes.data))
            return dict(vertex_idx=v, clusters=None, cluster_num=n, iters=it, rtn=rtn)
        v = np.zeros((B, 24), np.int32)
        cl = np.zeros((B, self.ccap, 3), np.int32)
        n, it, rtn = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        _check(_lib().direct_cluster_polygon_generation_batch(self.h, B, seeds.ctypes.data, int(itr_inflate_max),
                                                              int(itr_cluster_max), abi.MEM_HOST, v.ctypes.data,
                                                              cl.ctypes.data, n.ctypes.data, it.ctypes.data, rtn.ctypes.data))
        return dict(vertex_idx=v, clusters=[cl[b, :n[b]].copy() for b in range(B)], cluster_num=n, iters=it, rtn=rtn)

    def convex_test(self, inside, cand, cluster):
        """-> (can_clu [n], can_can packed lower triangle [n(n-1)/2], accept [n]), uint8 each"""
        inside = np.ascontiguousarray(inside, np.uint8)
        cand = np.ascontiguousarray(cand, np.int32).reshape(-1, 3)
        cluster = np.ascontiguousarray(cluster, np.int32).reshape(-1, 3)
        n = cand.shape[0]
        clu, acc = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        cc = np.zeros(max(n * (n - 1) // 2, 1), np.uint8)
        _check(_lib().direct_cluster_convex_test(self.h, inside.ctypes.data, n, cand.ctypes.data, cluster.shape[0],
                                                 cluster.ctypes.data, clu.ctypes.data, cc.ctypes.data, acc.ctypes.data))
        return clu, cc[:n * (n - 1) // 2], acc

    def hull_planes(self, resolution, map_lower, clusters=None, plane_capacity=256, vertex_capacity=1024, batch=None,
                    want=("planes", "plane_int", "vertices", "center"), num=None):
        """getConvexPoly's hull + Polyhedron::hrep + polyHrep2Utils (poly_utils.cpp:301-389, 127-206) for a batch of
        clusters.  clusters=None: those of the last polygon_generation, still on the device (`batch` of them);
        otherwise a list of [n][3] voxel-index arrays.  -> dict(planes: list of [P][4], plane_int, vertices: list of
        [V][3], center [B][3], degenerate, n_planes, n_vertices, rtn).  want: which of planes / plane_int / vertices /
        center are asked for; the C-ABI gets NULL for the others (no capacity applies to them) and the dict None.  num:
        cluster_num as the C-ABI is to see it, instead of the clusters' lengths (it clamps to [0, cluster_capacity])."""
        assert set(want) <= {"planes", "plane_int", "vertices", "center"}
        lower = np.ascontiguousarray(map_lower, np.float64)
        if clusters is not None:
            B = len(clusters)
            xyz = np.zeros((B, self.ccap, 3), np.int32)
            given, num = num, np.zeros(B, np.int32)
            for b, c in enumerate(clusters):
                c = np.ascontiguousarray(c, np.int32).reshape(-1, 3)
                assert len(c) <= self.ccap
                xyz[b, :len(c)] = c
                num[b] = len(c)
            if given is not None:
                num[:] = given
            px, pn = xyz.ctypes.data, num.ctypes.data
        else:
            B, px, pn = int(batch), None, None
        pl = np.zeros((B, plane_capacity, 4), np.float64)
        pi = np.zeros((B, plane_capacity, 4), np.int64)
        vt = np.zeros((B, vertex_capacity, 3), np.float64)
        ctr = np.zeros((B, 3), np.float64)
        npl, nv, deg, rtn = (np.zeros(B, np.int32) for _ in range(4))
        ptr = lambda a, k: a.ctypes.data if k in want else None
        _check(_lib().direct_cluster_hull_planes_batch(self.h, B, abi.MEM_HOST, px, pn, float(resolution), lower.ctypes.data,
                                                       int(plane_capacity), int(vertex_capacity), abi.MEM_HOST, ptr(pl, "planes"),
                                                       ptr(pi, "plane_int"), npl.ctypes.data, ptr(vt, "vertices"), nv.ctypes.data,
                                                       ptr(ctr, "center"), deg.ctypes.data, rtn.ctypes.data))
        cut = lambda a, n, cap, k: [a[b, :min(int(n[b]), cap)].copy() for b in range(B)] if k in want else None
        return dict(planes=cut(pl, npl, plane_capacity, "planes"), plane_int=cut(pi, npl, plane_capacity, "plane_int"),
                    vertices=cut(vt, nv, vertex_capacity, "vertices"), center=ctr if "center" in want else None,
                    degenerate=deg, n_planes=npl, n_vertices=nv, rtn=rtn)

    def grid_paths(self, starts, goals, path_capacity=4096, max_rounds=0, want_dist=False, mem="host"):
        """Optimal 26-connected voxel paths on the handle's map for a batch of (start, goal) voxel-index pairs
        (direct_cluster_grid_path_batch; stands where the reference calls gridPathFinder::AstarSearch).  -> dict(paths: list
        of [n][3] int32 arrays, start first (the first path_capacity voxels on GRID_PATH_OVERFLOW, empty without a path),
        path_len, path_cost, rtn, stats [B][2] (rounds, tile visits), dist [B][X*Y*Z] float64 or None).
        mem="device": the outputs stay on the device, as tensors in the C-ABI's own layout, for cube_corridors to read in place
        -> dict(path_xyz [B][path_capacity][3] int32, path_len, path_cost, rtn, stats)"""
        starts = np.ascontiguousarray(starts, np.int32).reshape(-1, 3)
        goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
        assert starts.shape == goals.shape
        B, cap = starts.shape[0], int(path_capacity)
        out, mem_abi, ptr = self._path_outputs(mem, B, B, cap, False, want_dist)
        _check(_lib().direct_cluster_grid_path_batch(self.h, B, starts.ctypes.data, goals.ctypes.data, cap, int(max_rounds), mem_abi,
                                                     *[ptr(k) for k in ("path_xyz", "path_len", "path_cost", "dist", "stats", "rtn")]))
        return out if mem == "device" else self._path_rows(out, cap)

    def _path_outputs(self, mem, n, n_field, cap, clear, want_dist):
        """The zeroed output set of a grid-path call with n paths on n_field fields (stats and dist are per field; path_d2 and
        path_min_d2 come with `clear`): NumPy arrays and a dist entry (None unless wanted) for mem="host", tensors in the C-ABI's
        layout for mem="device".  -> (dict, the C-ABI's memory kind, key -> address or None)"""
        assert mem in ("host", "device")
        if mem == "device":
            import torch
            assert not want_dist
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:%d" % self.device)
            i32, f64 = torch.int32, torch.float64
        else:
            z, i32, f64 = np.zeros, np.int32, np.float64
        out = dict(path_xyz=z((n, cap, 3), i32), path_len=z(n, i32), path_cost=z(n, f64), stats=z((n_field, 2), i32), rtn=z(n, i32))
        if clear:
            out.update(path_d2=z((n, cap), i32), path_min_d2=z(n, i32))
        if mem == "device":
            torch.cuda.current_stream(out["rtn"].device).synchronize()  # the handle's stream is not torch's
            return out, abi.MEM_DEVICE, lambda k: out[k].data_ptr() if k in out else None
        out["dist"] = np.zeros((n_field, int(np.prod(self.dims))), np.float64) if want_dist else None
        return out, abi.MEM_HOST, lambda k: None if out.get(k) is None else out[k].ctypes.data

    @staticmethod
    def _path_rows(out, cap):
        """Host outputs as the callers get them: path_xyz becomes paths, a list of each row's filled prefix, and so does path_d2."""
        n = [min(int(v), cap) for v in out["path_len"]]
        xyz = out.pop("path_xyz")
        out["paths"] = [xyz[b, :n[b]].copy() for b in range(len(n))]
        if "path_d2" in out:
            out["path_d2"] = [out["path_d2"][b, :n[b]].copy() for b in range(len(n))]
        return out

    def grid_paths_clear(self, starts, goals, min_d2=0, penalty=None, path_capacity=4096, max_rounds=0, want_dist=False, mem="host"):
        """grid_paths on the resident distance field (direct_cluster_grid_path_clear_batch; build_distance_field must have run since
        the map last changed): a move enters only voxels with stored D2 >= min_d2 (voxel^2), and entering voxel v costs the step
        weight plus penalty[D2[v]] (a float64 table, e.g. clearance_penalty_table; None: no penalty), two rounded additions in that
        order.  min_d2=0, penalty=None is grid_paths.  Returns what grid_paths returns for the same `mem`, plus
        path_d2 (host: a list of [n] int32 arrays beside paths; device: [B][path_capacity] int32), the stored D2 of each path
        voxel, and path_min_d2 [B], the minimum over the path without its start (DIST_NONE for a path of one voxel or none)."""
        starts = np.ascontiguousarray(starts, np.int32).reshape(-1, 3)
        goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
        assert starts.shape == goals.shape
        B, cap = starts.shape[0], int(path_capacity)
        pen = None if penalty is None else np.ascontiguousarray(penalty, np.float64).reshape(-1)
        par = GridPathClearIn(batch=B, path_capacity=cap, max_rounds=int(max_rounds), starts=starts.ctypes.data, goals=goals.ctypes.data,
                              min_d2=int(min_d2), n_penalty=0 if pen is None else len(pen), penalty=None if pen is None else pen.ctypes.data)
        out, par.mem, ptr = self._path_outputs(mem, B, B, cap, True, want_dist)
        o = GridPathClearOut(*[ptr(k) for k in abi.GRID_PATH_CLEAR_OUTPUTS])
        _check(_lib().direct_cluster_grid_path_clear_batch(self.h, C.addressof(par), C.addressof(o)))
        return out if mem == "device" else self._path_rows(out, cap)

    def grid_paths_fan(self, sources, goals, goal_src=None, min_d2=0, penalty=None, path_capacity=4096, max_rounds=0, want_dist=False,
                       mem="host"):
        """Many goals from few starts (direct_cluster_grid_path_fan_batch): ONE field per source, relaxed as far as its worst goal
        needs, and one read-back per goal - per goal the very bytes grid_paths (min_d2 <= 1 and penalty None or empty: neutral mode)
        or grid_paths_clear (anything else) returns for the pair (sources[goal_src[j]], goals[j]).  sources [S][3] with S <= max_batch,
        goals [n][3] with n unlimited, goal_src [n] (None: all goals belong to the one source).  Returns what grid_paths /
        grid_paths_clear return for the same `mem`, per goal (path_d2 and path_min_d2 in clear mode only), with stats [S][2] and
        dist [S][X*Y*Z] per SOURCE; mem="device" gives tensors in the C-ABI's layout, for cube_corridors to read in place."""
        sources = np.ascontiguousarray(sources, np.int32).reshape(-1, 3)
        goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
        gs = None if goal_src is None else np.ascontiguousarray(goal_src, np.int32).reshape(-1)
        assert gs is None or len(gs) == len(goals)
        S, n, cap = sources.shape[0], goals.shape[0], int(path_capacity)
        pen = None if penalty is None or len(penalty) == 0 else np.ascontiguousarray(penalty, np.float64).reshape(-1)
        clear = not (int(min_d2) <= 1 and pen is None)
        par = GridPathFanIn(n_src=S, n_goal=n, path_capacity=cap, max_rounds=int(max_rounds), sources=sources.ctypes.data,
                            goals=goals.ctypes.data, goal_src=None if gs is None else gs.ctypes.data, min_d2=int(min_d2),
                            n_penalty=0 if pen is None else len(pen), penalty=None if pen is None else pen.ctypes.data)
        out, par.mem, ptr = self._path_outputs(mem, n, S, cap, clear, want_dist)
        o = GridPathFanOut(*[ptr(k) for k in abi.GRID_PATH_FAN_OUTPUTS])
        _check(_lib().direct_cluster_grid_path_fan_batch(self.h, C.addressof(par), C.addressof(o)))
        return out if mem == "device" else self._path_rows(out, cap)

    def check_plans(self, n_seg, T, map_lower, resolution, bez=None, poly=None, depth=8, margin=0.0, t_from=None, outside_blocks=False, count=False):
        """Solved plans against the map the handle holds now (direct_cluster_plan_check_batch): for every plan whether the curve
        from t_from on is certified clear of occupied voxels, and otherwise the start time t_free of the first piece (of duration
        T_i / 2^depth) whose bounding box touches one - conservative: such a box need not mean that the curve enters the voxel.
        n_seg [B] int32, T [B][N], exactly one of bez / poly [B][N][18] (float32 or float64, one type for all three), t_from [B]
        float64 or None: NumPy arrays, or device tensors (then every output is a device tensor too).
        -> dict(status, verdict, t_free, first [B][2], hit_box [B][6], seg_first [B][N]); count=True adds the diagnostics unresolved
        (segment slots the first pass left to the deep pass) and box_tests, at the price of one atomic add per wave."""
        par = PlanCheckIn(depth=int(depth), outside_blocks=int(bool(outside_blocks)), resolution=float(resolution), margin=float(margin))
        i32, f64 = np.int32, np.float64
        _keep, out, ptr = self._plan_rows(par, n_seg, T, map_lower, bez, poly, t_from, (
            ("status", (), i32, 0), ("verdict", (), i32, 0), ("t_free", (), f64, 0), ("first", (2,), i32, 0), ("hit_box", (6,), i32, 0),
            ("seg_first", ("N",), i32, -1)))
        stats = np.zeros(2, np.int64)
        o = PlanCheckOut(*[ptr(a) for a in out.values()], stats.ctypes.data if count else None)  # the table's order is the struct's
        _check(_lib().direct_cluster_plan_check_batch(self.h, C.addressof(par), C.addressof(o)))
        if count:
            out.update(unresolved=int(stats[0]), box_tests=int(stats[1]))
        return out

    @staticmethod
    def _plan_rows(par, n_seg, T, map_lower, bez, poly, t_from, outputs):
        """The front of check_plans and plan_clearance, for NumPy arrays and device tensors alike: the inputs in the C-ABI's layout
        (float32 T keeps float32, anything else becomes float64, coefficients follow T), the zeroed outputs of the table `outputs`,
        rows of (name, shape behind [B] with "N" for n_seg_max, NumPy dtype, fill of a device tensor) in the output struct's order,
        and - written INTO `par` - the fields the two input structs share: mem, dtype, map_lower, batch, n_seg_max, n_seg, T, bez,
        poly, t_from.
        -> (the inputs, to be kept alive over the call; dict of outputs; array -> address)"""
        assert (bez is None) != (poly is None), "exactly one of bez and poly"
        coef = bez if poly is None else poly
        host = isinstance(T, np.ndarray) or not hasattr(T, "data_ptr")
        if host:
            T = np.asarray(T)
            real = np.float32 if T.dtype == np.float32 else np.float64
            T, coef = np.ascontiguousarray(T, real), np.ascontiguousarray(coef, real)
            n_seg = np.ascontiguousarray(n_seg, np.int32)
            tf = None if t_from is None else np.ascontiguousarray(t_from, np.float64)
            mk = lambda shape, dt, fill: np.zeros(shape, dt)
            ptr = lambda a: a.ctypes.data
            par.mem, par.dtype = abi.MEM_HOST, abi.F32 if real == np.float32 else abi.F64
        else:
            import torch
            real = torch.float32 if T.dtype == torch.float32 else torch.float64
            T, coef = T.to(real).contiguous(), coef.to(real).contiguous()
            n_seg = n_seg.to(torch.int32).contiguous()
            assert T.is_cuda and coef.is_cuda and n_seg.is_cuda
            tf = None if t_from is None else t_from.to(torch.float64).contiguous()
            mk = lambda shape, dt, fill: torch.full(shape, fill, dtype=getattr(torch, np.dtype(dt).name), device=T.device)
            ptr = lambda a: a.data_ptr()
            par.mem, par.dtype = abi.MEM_DEVICE, abi.F32 if real == torch.float32 else abi.F64
        B, N = T.shape
        out = {k: mk((B,) + tuple(N if s == "N" else s for s in shape), dt, fill) for k, shape, dt, fill in outputs}
        if not host:
            torch.cuda.current_stream(T.device).synchronize()  # the handle's stream is not torch's
        assert tuple(coef.shape) == (B, N, 18) and tuple(n_seg.shape) == (B,) and (tf is None or tuple(tf.shape) == (B,))
        par.map_lower = (C.c_double * 3)(*np.asarray(map_lower, np.float64).reshape(3))
        par.batch, par.n_seg_max = B, N
        par.n_seg, par.T = ptr(n_seg), ptr(T)
        par.bez, par.poly = (ptr(coef), None) if poly is None else (None, ptr(coef))
        par.t_from = None if tf is None else ptr(tf)
        return (n_seg, T, coef, tf), out, ptr

    def build_distance_field(self, cap_vox=0):
        """The exact squared Euclidean distance field of the map the handle holds now (direct_cluster_distance_field), in voxel
        units, resident on the handle until the map changes.  cap_vox > 0 stores min(D2, cap_vox^2) and bounds the work per voxel
        by cap_vox steps per axis.  -> dict(below_cap: voxels with a stored value below the cap, max_d2: the largest of them or -1)"""
        stats = np.zeros(2, np.int64)
        _check(_lib().direct_cluster_distance_field(self.h, int(cap_vox), stats.ctypes.data))
        return dict(below_cap=int(stats[0]), max_d2=int(stats[1]))

    def distance_field(self, out=None):
        """The stored field as an int32 array of shape dims (direct_cluster_get_distance_field); DIST_NONE on an empty map.  out: an
        int32 device tensor of shape dims to fetch into instead (returned)."""
        if out is None:
            d2 = np.zeros(self.dims, np.int32)
            _check(_lib().direct_cluster_get_distance_field(self.h, abi.MEM_HOST, d2.ctypes.data))
            return d2
        import torch
        assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == self.dims and out.is_contiguous()
        torch.cuda.current_stream(out.device).synchronize()  # the handle's stream is not torch's
        _check(_lib().direct_cluster_get_distance_field(self.h, abi.MEM_DEVICE, out.data_ptr()))
        return out

    def plan_clearance(self, n_seg, T, map_lower, resolution, bez=None, poly=None, depth=6, radius=0.0, t_from=None):
        """A certified lower bound, in metres, on each solved plan's distance to the occupied voxels, from the resident distance field
        (direct_cluster_plan_clearance_batch; build_distance_field must have run since the map last changed).  Inputs as check_plans;
        radius >= 0: from when on the plan is closer than that.  NumPy arrays, or device tensors (then every output is one too).
        -> dict(status, clearance, where [B][2], t_min, verdict, t_free, seg_clearance [B][N])"""
        par = PlanClearIn(depth=int(depth), resolution=float(resolution), radius=float(radius))
        i32, f64 = np.int32, np.float64
        _keep, out, ptr = self._plan_rows(par, n_seg, T, map_lower, bez, poly, t_from, (
            ("status", (), i32, 0), ("clearance", (), f64, 0), ("where", (2,), i32, 0), ("t_min", (), f64, 0), ("verdict", (), i32, 0),
            ("t_free", (), f64, 0), ("seg_clearance", ("N",), f64, float("nan"))))
        o = PlanClearOut(*[ptr(a) for a in out.values()])  # the table's order is the struct's
        _check(_lib().direct_cluster_plan_clearance_batch(self.h, C.addressof(par), C.addressof(o)))
        return out

    def cube_corridors(self, paths, path_len, map_lower, resolution, itr_inflate_max=1000, pop_back=True, seg_capacity=64, p_max=6,
                       dtype=np.float64):
        """The corridors of a batch of grid paths in the reference's is_cluster_on == false mode, every polytope the inflated cube
        of its seed voxel (direct_cluster_cube_corridor_batch): one call for all rows, planes in the optimiser's input layout.
        paths [B][path_capacity][3] int32 and path_len [B]: the outputs of the grid-path call, as NumPy arrays or as device tensors
        (grid_paths(mem="device")); every output is then of the same kind.  pop_back: corridorGeneration's walk (True) or
        corridorInsertGeneration's from an empty corridor (False).  dtype: float64, or float32 as one rounding of it.
        -> dict(n_seg [B], n_planes [B][S], planes [B][S][p_max][4], seeds [B][S][3], centers [B][S][3], cube_idx [B][S][6], rtn [B]),
        S = seg_capacity; entries from a row's n_seg on are zero"""
        return self._cube_corridors(_lib().direct_cluster_cube_corridor_batch, paths, path_len, map_lower, resolution, itr_inflate_max,
                                    pop_back, seg_capacity, p_max, dtype)

    def cube_corridors_clear(self, paths, path_len, map_lower, resolution, min_d2, itr_inflate_max=1000, pop_back=True, seg_capacity=64,
                             p_max=6, dtype=np.float64):
        """cube_corridors on the resident distance field (direct_cluster_cube_corridor_clear_batch): a cube stops at voxels whose
        stored D2 is below min_d2 (voxel^2, the floor of grid_paths_clear / grid_paths_fan), so every voxel of a cube but its seed
        has D2 >= min_d2.  min_d2 <= 1 is cube_corridors and needs no field; min_d2 >= 2 needs build_distance_field() after the
        last change of the map and a floor not above the field's cap2.  Arguments, kinds and result as cube_corridors, plus
        info [2] int64 (NumPy): info[0] 1 if the call built a floor table, 0 if it reused one (two stay resident, least recently
        used replaced) or ran in neutral mode; info[1] the voxels below the floor."""
        info = np.zeros(2, np.int64)
        fn = _lib().direct_cluster_cube_corridor_clear_batch
        out = self._cube_corridors(lambda h, par, o: fn(h, par, int(min_d2), o, info.ctypes.data), paths, path_len, map_lower, resolution,
                                   itr_inflate_max, pop_back, seg_capacity, p_max, dtype)
        out["info"] = info
        return out

    def cluster_corridors(self, paths, path_len, map_lower, resolution, itr_inflate_max=1000, itr_cluster_max=50, pop_back=True,
                          seg_capacity=64, p_max=64, dtype=np.float64):
        """The corridors of a batch of grid paths in the mode the reference ships, is_cluster_on == true: every polytope the hull of
        the voxel cluster grown from its seed (direct_cluster_corridor_batch).  The walk runs on the device; per round the due seeds
        are de-duplicated by voxel and generated in chunks of max_batch; per row the result is, bit for bit, the lock-step walk over
        polygon_generation + hull_planes.  Arguments, kinds (NumPy arrays or device tensors) and layouts as cube_corridors;
        itr_cluster_max=0 gives cubes.  The call invalidates resident clusters.
        -> dict(n_seg [B], n_planes [B][S], planes [B][S][p_max][4], seeds [B][S][3], centers [B][S][3], rtn [B] (CLUSTER_CORRIDOR_*),
        stats: dict(rounds, due_seeds, unique_seeds, pops)); entries from a row's n_seg on are zero"""
        stats = np.zeros(4, np.int64)
        par = ClusterCorridorIn(itr_cluster_max=int(itr_cluster_max))
        fn = _lib().direct_cluster_corridor_batch
        out = self._cube_corridors(lambda h, p, o: fn(h, p, o, stats.ctypes.data), paths, path_len, map_lower, resolution, itr_inflate_max,
                                   pop_back, seg_capacity, p_max, dtype, par=par, out_type=ClusterCorridorOut, keys=abi.CLUSTER_CORRIDOR_OUTPUTS)
        out["stats"] = {k: int(v) for k, v in zip(abi.CLUSTER_CORRIDOR_STATS, stats)}
        return out

    def _cube_corridors(self, call, paths, path_len, map_lower, resolution, itr_inflate_max, pop_back, seg_capacity, p_max, dtype,
                        par=None, out_type=CubeCorridorOut, keys=abi.CUBE_CORRIDOR_OUTPUTS):
        """the corridor calls: call(handle, address of the input struct, address of the output struct) -> status.  par: an input
        struct with the call's own fields set (None: CubeCorridorIn); out_type / keys: its output struct and that struct's arrays"""
        lower = np.asarray(map_lower, np.float64).reshape(3)
        f32 = np.dtype(dtype) == np.float32
        par = CubeCorridorIn() if par is None else par
        par.itr_inflate_max, par.pop_back, par.seg_capacity, par.p_max = int(itr_inflate_max), int(bool(pop_back)), int(seg_capacity), int(p_max)
        par.plane_dtype, par.resolution, par.map_lower = abi.F32 if f32 else abi.F64, float(resolution), (C.c_double * 3)(*lower)
        S, P = int(seg_capacity), int(p_max)
        if isinstance(paths, np.ndarray) or not hasattr(paths, "data_ptr"):
            paths, path_len = np.ascontiguousarray(paths, np.int32), np.ascontiguousarray(path_len, np.int32)
            B = paths.shape[0]
            real = np.float32 if f32 else np.float64
            z = lambda shape, dt: np.zeros(shape, dt)
            ptr = lambda a: a.ctypes.data
            par.mem_in = mem = abi.MEM_HOST
        else:
            import torch
            paths, path_len = paths.to(torch.int32).contiguous(), path_len.to(torch.int32).contiguous()
            assert paths.is_cuda and path_len.is_cuda
            B = paths.shape[0]
            real = torch.float32 if f32 else torch.float64
            z = lambda shape, dt: torch.zeros(shape, dtype={np.int32: torch.int32}.get(dt, dt), device=paths.device)
            torch.cuda.current_stream(paths.device).synchronize()  # the handle's stream is not torch's
            ptr = lambda a: a.data_ptr()
            par.mem_in = mem = abi.MEM_DEVICE
        assert paths.ndim == 3 and paths.shape[2] == 3 and tuple(path_len.shape) == (B,)
        par.batch, par.path_capacity = B, int(paths.shape[1])
        par.path_xyz, par.path_len = ptr(paths), ptr(path_len)
        out = dict(n_seg=z(B, np.int32), n_planes=z((B, S), np.int32), planes=z((B, S, P, 4), real), seeds=z((B, S, 3), real),
                   centers=z((B, S, 3), real), cube_idx=z((B, S, 6), np.int32), rtn=z(B, np.int32))
        out = {k: out[k] for k in keys}
        o = out_type(mem, 0, *[ptr(out[k]) for k in keys])
        _check(call(self.h, C.addressof(par), C.addressof(o)))
        return out

    def build_free_components(self, min_d2=0):
        """The 26-connected components of the enterable voxels of the map the handle holds now (direct_cluster_free_components):
        a voxel is enterable when its byte is 0 and, for min_d2 > 1, its stored D2 is at least min_d2 (build_distance_field must
        then have run since the map last changed) - the graph grid_paths / grid_paths_clear / grid_paths_fan move on.  Labels and
        sizes stay resident on the handle until the map (or, with a floor, the field) changes.
        -> dict(enterable, components, largest: size of the largest component, largest_label: its label or -1)"""
        stats = np.zeros(4, np.int64)
        _check(_lib().direct_cluster_free_components(self.h, int(min_d2), stats.ctypes.data))
        return dict(enterable=int(stats[0]), components=int(stats[1]), largest=int(stats[2]), largest_label=int(stats[3]))

    def free_components(self, mem="host"):
        """-> (label, size), int32 of shape dims (direct_cluster_get_free_components): label is -1 on a voxel that is not enterable,
        else the smallest linear index of its component; size the component's voxel count, else 0.  mem="device": tensors."""
        assert mem in ("host", "device")
        if mem == "host":
            label, size = np.zeros(self.dims, np.int32), np.zeros(self.dims, np.int32)
            _check(_lib().direct_cluster_get_free_components(self.h, abi.MEM_HOST, label.ctypes.data, size.ctypes.data, None))
            return label, size
        import torch
        label, size = (torch.zeros(self.dims, dtype=torch.int32, device="cuda:%d" % self.device) for _ in range(2))
        torch.cuda.current_stream(label.device).synchronize()  # the handle's stream is not torch's
        _check(_lib().direct_cluster_get_free_components(self.h, abi.MEM_DEVICE, label.data_ptr(), size.data_ptr(), None))
        return label, size

    def free_components_floor(self):
        """the normal form (<= 1 -> 0) of the min_d2 the resident labels were built with"""
        v = C.c_int32(-1)
        _check(_lib().direct_cluster_get_free_components(self.h, abi.MEM_HOST, None, None, C.addressof(v)))
        return v.value

    def reachable(self, starts, goals, min_d2=0, mem="host"):
        """Which code grid_paths / grid_paths_clear / grid_paths_fan would return for each (start, goal) pair, from the resident
        labels alone (direct_cluster_reachable_batch): GRID_PATH_OK (an OVERFLOW there is OK here), GRID_PATH_NO_PATH or
        GRID_PATH_BAD_ENDPOINT.  starts, goals [n][3] int32, n unlimited: NumPy arrays or device tensors (one kind for both);
        min_d2 must be the floor build_free_components ran with.  mem: where the outputs go ("host": NumPy, "device": tensors).
        -> (rtn [n], goal_label [n], goal_size [n]): the goal's component and its voxel count, -1 and 0 for a goal that is
        outside the map or not enterable - to drop goals in pockets too small to matter."""
        assert mem in ("host", "device")
        if isinstance(starts, np.ndarray) or not hasattr(starts, "data_ptr"):
            starts = np.ascontiguousarray(starts, np.int32).reshape(-1, 3)
            goals = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
            mem_in, ps, pg = abi.MEM_HOST, starts.ctypes.data, goals.ctypes.data
        else:
            import torch
            starts, goals = starts.to(torch.int32).contiguous().reshape(-1, 3), goals.to(torch.int32).contiguous().reshape(-1, 3)
            assert starts.is_cuda and goals.is_cuda
            torch.cuda.current_stream(starts.device).synchronize()  # the handle's stream is not torch's
            mem_in, ps, pg = abi.MEM_DEVICE, starts.data_ptr(), goals.data_ptr()
        assert tuple(starts.shape) == tuple(goals.shape)
        n = int(starts.shape[0])
        if mem == "host":
            out = [np.zeros(n, np.int32) for _ in abi.REACHABLE_OUTPUTS]
            ptrs = [a.ctypes.data for a in out]
        else:
            import torch
            out = [torch.zeros(n, dtype=torch.int32, device="cuda:%d" % self.device) for _ in abi.REACHABLE_OUTPUTS]
            torch.cuda.current_stream(out[0].device).synchronize()
            ptrs = [a.data_ptr() for a in out]
        par = ReachableIn(n=n, mem_in=mem_in, min_d2=int(min_d2), starts=ps, goals=pg)
        o = ReachableOut(abi.MEM_HOST if mem == "host" else abi.MEM_DEVICE, 0, *ptrs)
        _check(_lib().direct_cluster_reachable_batch(self.h, C.addressof(par), C.addressof(o)))
        return tuple(out)

    def set_stream(self, hip_stream):
        _check(_lib().direct_cluster_set_stream(self.h, C.c_void_p(hip_stream)))

    def last_ms(self):
        ms = C.c_float()
        _check(_lib().direct_cluster_last_ms(self.h, C.addressof(ms)))
        return ms.value
