/*
 * direct_cluster.h -- C-ABI of the MI355X-native corridor-cluster generator: the step that
 * produces the polytopes the DDP path consumes.  Replaces, for a BATCH of seed voxels on one voxel map,
 *
 *   void cudaPolytopeGeneration::polygonGeneration(vector<int>& x, vector<int>& y, vector<int>& z)
 *       polyhedron_generator/include/polyhedron_generator/cluster_server_cpu.h:61   (shipped CPU build)
 *       polyhedron_generator/src/cluster_server_cpu.cpp:394-528
 *   with paramSet / setObs / mapClear (cluster_server_cpu.cpp:8-46, 83-120) for the map,
 *
 * whose inner loops are cubeInflation_cpu (:257-293), polytopeCluster_cpu (:295-392) and serialConvexTest
 * (cluster_engine_cpu.cpp:31-136); the reference's optional CUDA twins are paraCubeInflation / paraConvexTest /
 * paraResultCheck (cluster_engine.cu:37-350).  RESULTS ARE THOSE OF THE SHIPPED CPU BUILD, bit for bit: the same
 * cluster voxels in the same order (the CUDA twins use a different DDA - double precision, different termination
 * order - and are not what poly_utils.h:13-14 links).  The caller is polyhedronGenerator::getConvexPoly
 * (global_planner/src/utils/poly_utils.cpp:285-299), which passes ONE seed voxel per call; a batch here is many
 * such calls (every seed along an A* path, or many paths) on the same map.
 *
 * Voxel (x, y, z) lives at index x * max_y * max_z + y * max_z + z (cluster_server_cpu.cpp:30).  Map bytes are
 * 0 (free) or 1 (obstacle), as setObs / setFr write them.  Plain pointers and sizes only.
 */
#ifndef DIRECT_CLUSTER_H_
#define DIRECT_CLUSTER_H_

#include <stddef.h>
#include <stdint.h>

#include "direct_ddp.h" /* direct_status_t, direct_mem_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t device;             /* HIP device ordinal */
  int32_t max_x, max_y, max_z; /* paramSet's max_x_id, max_y_id, max_z_id (voxels per axis) */
  int32_t max_batch;          /* seeds per call */
  int32_t cluster_capacity;   /* voxels per cluster (_cluster_buffer_size: 50000 in the CPU build) */
  int32_t candidate_capacity; /* candidates per round (_candidate_buffer_size: 10000) */
  int32_t reserved;
} direct_cluster_config_t;

typedef struct direct_cluster_handle_s* direct_cluster_handle_t;

direct_status_t direct_cluster_create(const direct_cluster_config_t* cfg, direct_cluster_handle_t* out);
direct_status_t direct_cluster_destroy(direct_cluster_handle_t h);
const char* direct_cluster_last_error(void);

/* mapClear + setObs for every obstacle voxel + mapUpload: the whole occupancy grid at once.
 * map_data[max_x*max_y*max_z] in memory kind `mem`. */
direct_status_t direct_cluster_set_map(direct_cluster_handle_t h, int32_t mem, const uint8_t* map_data);

/* ---- the map from a point cloud: the stage in front of everything (cloud -> map -> grid path -> corridor) ----------
 * Builds the resident map from the points a sensor delivers, where the reference runs rcvPointCloudCallBack
 * (global_planner/src/teach_repeat_planner.cpp:523-581, "TRP") on one thread.  The map is the reference's, bit for bit:
 *   Steps      s = (int)round(cloud_margin * inv), inv = 1.0 / resolution computed once (TRP:537, 1201), in x and y;
 *              s_z = max(1, s / 2) in integer division in z (TRP:538).  cloud_margin = 0.0, the shipped launch file's
 *              map_margin (global_planner.launch:34), still inflates by one voxel up and down in z.
 *   Inflation  acts on COORDINATES, not on voxels: for every point and every offset (kx, ky, kz) of the
 *              (2s+1)^2 x (2s_z+1) box the coordinate (double)p + (double)k * resolution is formed per axis (TRP:548-550:
 *              p a float promoted to double, two roundings, no fused multiply-add) and quantised as
 *              int((coord - lower) * inv).  A float32 point on a voxel face can land in either neighbour after the shift;
 *              this is NOT "the point's voxel dilated by a box".
 *   Border     the reference keeps two maps that disagree there:
 *              DIRECT_MAP_BORDER_CLAMP  the polytope generator's: setObs(coord2gridIndex(coord)) (TRP:553, 557;
 *                utils/a_star.h:141-149), index min(max(int(q), 0), size - 1) per axis: a point outside the map marks
 *                border voxels.  This is the map polygon_generation_batch / hull_planes_batch stand on in the reference.
 *              DIRECT_MAP_BORDER_DROP   the path finder's: setObs(x, y, z) (TRP:556; utils/a_star.cpp:74-85) discards a
 *                coordinate outside [map_lower, map_upper) along any axis.  This is the map AstarSearch runs on.
 *   Defined here, undefined in the reference:
 *              (1) int(double) of a NaN or an out-of-range value: a point with ANY non-finite coordinate contributes
 *                  nothing and is counted in stats[1]; a finite coordinate far outside is compared against the range before
 *                  any conversion (CLAMP: the border voxel; DROP: discarded).
 *              (2) in the path finder's setObs a coordinate in [size * resolution + map_lower, map_upper) passes the range
 *                  test and indexes one past the array (49.95 .. 50 at the launch file's values): DROPPED here.
 * The bytes written are 1; every writer of a voxel writes the same byte, so the map depends neither on the order of the
 * points nor on the launch shape.  The summed-area table of the obstacles is rebuilt by the same code as in
 * direct_cluster_set_map, and the call has set_map's effect on everything else the handle holds (resident clusters stay).
 * xyz[n_points][stride] floats in memory kind `mem` (DIRECT_MEM_HOST or DIRECT_MEM_DEVICE); the map's size in voxels is the
 * handle's.  stats (host, may be NULL): [0] points read, [1] points skipped as non-finite, [2] (point, offset) triples
 * dropped by BORDER_DROP (0 under CLAMP), [3] voxels with byte 1 after the call.
 * DIRECT_ERR_INVALID: null handle or parameters; n_points < 0; xyz == NULL with n_points > 0; resolution <= 0 or not
 * finite; cloud_margin < 0 or not finite; map_lower (and map_upper under DROP) not finite; stride other than 3 or 4; unknown
 * border, mode or mem.  DIRECT_ERR_UNSUPPORTED: s above 1024.  n_points == 0 with REPLACE gives an empty map, which IS a map.
 * Runs on the handle's stream and synchronises before it returns; direct_cluster_last_ms covers the clear, the kernel and
 * the table (not the copy of a host cloud). */
#define DIRECT_MAP_BORDER_CLAMP 0  /* the polytope generator's map: coord2gridIndex clamps (TRP:553, 557) */
#define DIRECT_MAP_BORDER_DROP  1  /* the path finder's map: setObs(x, y, z) discards (a_star.cpp:74-85) */
#define DIRECT_MAP_REPLACE 0       /* mapClear first */
#define DIRECT_MAP_ADD     1       /* keep what the handle holds; a handle without a map starts empty, as after paramSet */
typedef struct {
  double map_lower[3], map_upper[3];   /* map_upper is read by BORDER_DROP only */
  double resolution, cloud_margin;
  int32_t border, mode;
  int32_t stride;                      /* floats per point: 3, or 4 for a pcl::PointXYZ buffer as it lies in memory */
  int32_t reserved;
} direct_map_cloud_t;
direct_status_t direct_cluster_map_from_cloud(direct_cluster_handle_t h, const direct_map_cloud_t* p, int64_t n_points,
                                              int32_t mem, const float* xyz, int64_t* stats /* host [4], may be NULL */);
/* The handle's map, map_data[max_x*max_y*max_z] in memory kind `mem`; DIRECT_ERR_INVALID without a map. */
direct_status_t direct_cluster_get_map(direct_cluster_handle_t h, int32_t mem, uint8_t* map_data);

/* Return codes per seed (the reference has none: it writes past its buffers instead). */
#define DIRECT_CLUSTER_OK 0
#define DIRECT_CLUSTER_OVERFLOW 1  /* cluster_capacity / candidate_capacity exceeded: the cluster is incomplete (see below) */
#define DIRECT_CLUSTER_BAD_SEED 2  /* seed voxel outside the map */

/* polygonGeneration for `batch` seeds (host array seeds[batch][3]).  itr_inflate_max / itr_cluster_max as given to
 * paramSet with is_cluster_on (is_cluster_on == false is (1000, 0)).  Outputs in memory kind `mem`, any may be NULL:
 *   vertex_idx[batch][24]       the inflated cube (cluster_server_cpu.cpp:48-60 layout: x 0..7, y 8..15, z 16..23)
 *   cluster_xyz[batch][cluster_capacity][3]   cluster voxels in the reference's order
 *   cluster_num[batch], cluster_iters[batch] (completed rounds of polytopeCluster_cpu), rtn[batch] (codes above)
 * A row that ends with DIRECT_CLUSTER_OVERFLOW (the cube's surface, or a round's accepted candidates, would pass
 * cluster_capacity; a round has more candidates than candidate_capacity) keeps its vertex_idx, and cluster_num <= cluster_capacity
 * voxels that are a PREFIX of the cluster the reference would build, in its order.  When the cube's surface alone passes
 * cluster_capacity the prefix is the first cluster_capacity voxels of the surface and no round has run; otherwise how long a prefix
 * is not specified (the surface and the rounds completed before the overflow at least, the capacity at most).  cluster_iters counts
 * the completed rounds only, and the row is not
 * a cluster to build a hull from (direct_cluster_hull_planes_batch gives a resident row like it no planes).  Codes are per row: the
 * other rows of the batch are what they would be alone. */
direct_status_t direct_cluster_polygon_generation_batch(direct_cluster_handle_t h, int32_t batch, const int32_t* seeds,
                                                        int32_t itr_inflate_max, int32_t itr_cluster_max, int32_t mem,
                                                        int32_t* vertex_idx, int32_t* cluster_xyz, int32_t* cluster_num,
                                                        int32_t* cluster_iters, int32_t* rtn);

/* ---- kernel-level entry point (parity tests against the reference's own serialConvexTest) ----------------------
 * One convex test round on caller-provided state: for every candidate i
 *   can_clu[i]  = serialConvexTest(candidate i, cluster[0..n_cluster), inside_data, map)      (uint8 0/1)
 *   can_can[i*(i-1)/2 + j], j < i  = the same ray test from candidate i towards candidate j alone
 *                 (the packed lower triangle of paraResultCheck, cluster_engine.cu:37-67; may be NULL)
 *   accept[i]   = can_clu[i] && for all j < i with accept[j]: can_can[i][j]     -- what polytopeCluster_cpu's
 *                 sequential loop decides (cluster_server_cpu.cpp:360-384), since serialConvexTest is an AND over
 *                 targets and accepted candidates join the cluster at once (may be NULL)
 * All arrays are HOST memory; inside_data is the reference's per-voxel flag array.
 * The call uses the handle's cluster storage: it INVALIDATES the clusters a preceding
 * direct_cluster_polygon_generation_batch left resident (a following direct_cluster_hull_planes_batch with
 * cluster_xyz == NULL fails with DIRECT_ERR_INVALID until the next generation). */
direct_status_t direct_cluster_convex_test(direct_cluster_handle_t h, const uint8_t* inside_data, int32_t n_candidate,
                                           const int32_t* candidate_xyz, int32_t n_cluster, const int32_t* cluster_xyz,
                                           uint8_t* can_clu, uint8_t* can_can, uint8_t* accept);

/* ---- hull -> planes (the tail of SURVEY.md 8f-4): cluster voxels -> the polytope the DDP path consumes ---------
 * Replaces, for a batch of clusters, what polyhedronGenerator does with the result of polygonGeneration
 * (global_planner/src/utils/poly_utils.cpp):
 *   getConvexPoly   :301-389  point set (voxel centres; the eight corners of every voxel when checkDegeneratePoly
 *                             :236-273 finds the cluster flat along an axis), third_party/quickhull, vertex buffer
 *   Polyhedron::hrep (eigen-cdd / cddlib), call sites :404-449, :470-480   V-rep -> A x <= b
 *   polyHrep2Utils  :127-206  unit normals pointing outwards, plane (a, b, c, d) with a x + b y + c z + d <= 0 inside,
 *                             axis-aligned faces of a solid cluster moved out by half a voxel, centre
 * All of the reference's points lie on the half-voxel lattice q = 2 index + 1 (+/- 1 for corners), world coordinate
 * x = q * resolution / 2 + map_lower, so the hull is computed in exact integer arithmetic: the planes are THE facet
 * planes the two floating-point libraries approximate.  Not reproducible and therefore defined here: the ORDER of the
 * rows (cdd's; here ascending (nx, ny, nz, K) of the primitive integer normal) and the per-plane vertex behind the
 * centre (an argmin over residuals that are all ~1e-16; here the first corner, in cluster order, on the plane).
 * Vertices are the corners of the hull in cluster order (quickhull's vertex buffer may also hold boundary points that
 * are not corners; cdd's H-rep does not depend on them).
 * EXTENT: no limit beyond the map's (1024 voxels per axis).  With D the diameter of a cluster in lattice units
 * (D < 2^11.8) the orientation tests stay below 2^60; the one product that reaches D^6 - it overflowed 64 bits from a
 * width of 725 voxels on - is carried in 128 bits (hull_core.h).  A cluster never comes back DIRECT_HULL_OK with planes
 * other than its hull's.
 *
 * cluster_xyz == NULL: the clusters of the last polygon_generation_batch, still resident on the device (no copy of
 * the voxels in either direction; `batch` may not exceed that call's, and a seed whose generation did not end with
 * DIRECT_CLUSTER_OK has no usable cluster: DIRECT_HULL_OVERFLOW / DIRECT_HULL_FLAT).  Otherwise
 * cluster_xyz[batch][cluster_capacity][3] / cluster_num[batch] in memory kind mem_in REPLACE them in the handle's storage
 * (a later call with cluster_xyz == NULL needs a new generation first); every voxel must lie inside the map.  Outputs in memory kind `mem`, any may be NULL:
 *   planes[batch][plane_capacity][4] (double), plane_int[batch][plane_capacity][4] (int64: primitive normal and
 *   offset on the lattice, n . q + K <= 0), n_planes[batch], vertices[batch][vertex_capacity][3], n_vertices[batch],
 *   center[batch][3], degenerate[batch] (checkDegeneratePoly), rtn[batch] (codes below). */
#define DIRECT_HULL_OK 0
#define DIRECT_HULL_OVERFLOW 1 /* more planes / vertices than the capacity of an output that was asked for, more than 2048 line-extreme points or 8192 plane reports of hull edges, more than 2048 planes with `center` asked for, or a resident cluster whose generation overflowed */
#define DIRECT_HULL_BAD_VOXEL 2 /* a caller-provided voxel lies outside the map [0, max_x) x [0, max_y) x [0, max_z): nothing is computed for the cluster */
#define DIRECT_HULL_FLAT 3     /* empty cluster, or the points do not span three dimensions (the reference's cdd call fails) */
direct_status_t direct_cluster_hull_planes_batch(direct_cluster_handle_t h, int32_t batch, int32_t mem_in,
                                                 const int32_t* cluster_xyz, const int32_t* cluster_num, double resolution,
                                                 const double* map_lower, int32_t plane_capacity, int32_t vertex_capacity,
                                                 int32_t mem, double* planes, int64_t* plane_int, int32_t* n_planes,
                                                 double* vertices, int32_t* n_vertices, double* center, int32_t* degenerate,
                                                 int32_t* rtn);

/* ---- grid paths: the stage in front of the corridor (map -> grid path -> corridor) -------------------------------
 * Shortest 26-connected voxel paths for a BATCH of (start, goal) queries on the map of direct_cluster_set_map.  Stands where
 * the reference calls gridPathFinder::AstarSearch (global_planner/src/utils/a_star.cpp:179-280, from
 * teach_repeat_planner.cpp:163-169), on the reference's own graph with the reference's own cost arithmetic, but it returns
 * the OPTIMAL path: the reference multiplies its heuristic by a tie_breaker > 1 and depends on its expansion order, so its
 * path costs this much or more and is not reproduced.
 *   Graph   the 26 neighbours of a voxel (a_star.cpp:224-234).  A move goes INTO a voxel that lies inside the map
 *           (:236-240) and whose map byte is 0 (:242-246).  No corner-cutting rule, as in the reference.  The start
 *           voxel's own byte is not looked at (the reference expands it regardless, :194-198).
 *   Cost    d(start) = 0, d(v) = min over the neighbours u of fl(d(u) + w), w = sqrt(dx^2 + dy^2 + dz^2) in {1.0, sqrt(2.0),
 *           sqrt(3.0)} as doubles, one rounded double addition per move: gScore's arithmetic (:252-254), folded from the
 *           START.  This is the cost a heap Dijkstra (or an admissible A*) with the same additions returns, bit for bit.
 *   Path    path_cost = d(goal).  The path is read backwards from the goal: the predecessor of v is the first neighbour u,
 *           in ascending (dx, dy, dz) lexicographic order from (-1, -1, -1), that is in the graph and has
 *           fl(d(u) + w) == d(v) as doubles.  It is emitted start first, goal last; the left-to-right double sum of its
 *           step weights equals path_cost to the bit.
 * starts / goals are HOST arrays [batch][3] of voxel indices; batch <= max_batch; path_capacity > 0 (it decides OVERFLOW
 * whether path_xyz is asked for or not).  Outputs in memory kind `mem` (DIRECT_MEM_HOST or DIRECT_MEM_DEVICE; anything else is
 * DIRECT_ERR_INVALID), any may be NULL:
 *   path_xyz[batch][path_capacity][3], path_len[batch] (voxels on the path: the length NEEDED, also on overflow),
 *   path_cost[batch], rtn[batch] (codes below, per query: other queries are unaffected),
 *   dist[batch][max_x*max_y*max_z]  the field d: exact wherever the true distance is <= path_cost (for NO_PATH: the whole
 *           connected component of the start); elsewhere any value >= the true distance, +inf included (the search is
 *           pruned by the goal's current value).  Obstacle voxels hold +inf (an occupied start holds its 0).
 *   stats[batch][2]  rounds in which the query had an active tile, tile visits: diagnostic, NOT deterministic.
 * path_xyz, path_len, path_cost, rtn and dist where it is exact do not depend on the launch shape: one call of 64, two
 * calls of 32 and a permuted batch give identical bytes.
 * Method: a label-correcting relaxation over 8^3 tiles, one kernel launch per round; max_rounds bounds the rounds
 * (0: the library's default, 2 * (number of tiles) + 64) and a query still changing then ends with ROUND_LIMIT.
 * The call owns a workspace of its own, allocated by the first call, never shrunk and freed in direct_cluster_destroy:
 * the field in double, 8 B x voxels x max_batch (0.82 GB at 64 x 1.6 M voxels), plus one activity byte per tile and query
 * (twice) and 4 B x path_capacity per query for the read-back.  It does NOT invalidate the clusters a preceding
 * direct_cluster_polygon_generation_batch left resident.  direct_cluster_last_ms covers it, direct_cluster_set_stream is
 * honoured. */
#define DIRECT_GRID_PATH_OK 0
#define DIRECT_GRID_PATH_NO_PATH 1      /* goal occupied and != start, or not connected: path_len 0, path_cost +inf */
#define DIRECT_GRID_PATH_BAD_ENDPOINT 2 /* start or goal outside the map: nothing is computed, path_len 0, path_cost NaN */
#define DIRECT_GRID_PATH_OVERFLOW 3     /* path longer than path_capacity: path_len is the needed length, path_cost is valid, path_xyz holds the first path_capacity voxels */
#define DIRECT_GRID_PATH_ROUND_LIMIT 4  /* max_rounds reached with tiles still active: no path (path_len 0, path_cost NaN); never a hang */
/* start == goal is OK with length 1 and cost 0 (a_star.cpp:208-218), whatever the voxel's byte. */
direct_status_t direct_cluster_grid_path_batch(direct_cluster_handle_t h, int32_t batch, const int32_t* starts,
                                               const int32_t* goals, int32_t path_capacity, int32_t max_rounds, int32_t mem,
                                               int32_t* path_xyz, int32_t* path_len, double* path_cost, double* dist,
                                               int32_t* stats, int32_t* rtn);

/* ---- plans against the resident map: the step after a sensor update (no reference counterpart) --------------------
 * Is each of these solved plans still clear of the map the handle holds NOW, and if not, until when is it safe?  The audit
 * (direct_traj_audit_batch) judges a plan against the corridor it was solved in, which describes the map as it was; this call
 * judges it against the voxels, with box tests on the handle's summed-area table alone: no root finding, no tolerance, every
 * output a pure function of the inputs and bit for bit reproducible.
 * batch, n_seg_max, mem, n_seg, T and exactly one of bez / poly: meaning, layouts and row validity as in direct_eval_in_t
 * (include/direct_ddp.h, items 1 and 6 there); dtype (direct_dtype_t) is the storage type of T, bez and poly - the cluster
 * handle has none of its own.  map_lower and resolution place the voxels, as in direct_cluster_map_from_cloud;
 * inv = 1.0 / resolution is computed once on the host.  All arithmetic is double with contraction off, written with plain
 * * and + (no fma), so that a NumPy restatement performs the same operations.  For a valid row of n segments:
 *   1. Control points in metres, per segment and axis.  From bez: P_j = T * c_j.  From poly: P_j = sum_{m=0..j} w[j][m] *
 *      (a_m * Tm), summed with ascending m, w[j][m] = (double)C(j,m) / (double)C(5,m), Tm by repeated multiplication
 *      (T^0 = 1, T^m = T^(m-1) * T).
 *   2. Leaves.  Leaf k (0 <= k < 2^D, D = depth) of a segment is the result of D de Casteljau halvings of its six points, every
 *      new point (a + b) * 0.5; at step l the half is chosen by bit D-1-l of k (0: left, 1: right).  It spans the plan time
 *      [S_i + (k * 2^-D) * T_i, S_i + ((k+1) * 2^-D) * T_i] - the factor exact, the product rounded, then the sum, S the
 *      evaluation's cumulative sum; the end of a segment's last leaf is S_(i+1) to the bit.
 *   3. Box of a leaf, per axis a: q_lo = ((min_j P_j[a] - margin) - map_lower[a]) * inv, q_hi = ((max_j P_j[a] + margin) -
 *      map_lower[a]) * inv; the index is size[a] when q >= size[a], -1 when q < 0 (or q is NaN), else (int)q - compared before it
 *      is converted: the voxel int((coord - lower) * inv) the map builder would have put the coordinate in.  The box LEAVES THE
 *      MAP when any i_lo == -1 or any i_hi == size.  It is OCCUPIED when a voxel with byte 1 lies in its intersection with the
 *      map (an empty intersection is not occupied).  It is BLOCKED when it is occupied, or when outside_blocks is set and it
 *      leaves the map.
 *   4. A leaf is judged iff its end time is > t_from[b] (t_from == NULL: every leaf).
 *   5. Outputs (any but status may be NULL):
 *      status [batch]           0 or -1 (required)
 *      verdict [batch]          0: every judged leaf's box is unblocked - the continuous curve from t_from on lies in free voxels
 *                               (inside the map too when outside_blocks is set); otherwise the facts about the first blocked
 *                               judged leaf: 1 it is occupied, 2 it leaves the map, 3 both (bit 1 is reported whether or not
 *                               outside_blocks is set); DIRECT_PLAN_CHECK_INVALID for an invalid row
 *      t_free [batch] (double)  the start time of the first blocked judged leaf, in (segment, k) order; S_n when the verdict is
 *                               0; 0 for an invalid row.  From t_from up to t_free the plan is certified clear: the time to hand
 *                               to direct_traj_eval_batch for the start state of a replan.
 *      first [batch][2]         that segment and leaf; (-1, -1) when there is none
 *      hit_box [batch][6]       that leaf's i_lo[3], i_hi[3]; all -1 when there is none
 *      seg_first [batch][n_seg_max]  the first blocked judged leaf of each segment, or -1.  Entries past n_seg are untouched in
 *                               device memory and -1 in host memory; the first min(n_seg, n_seg_max) of an invalid row are -1.
 *      stats (HOST, [2])        diagnostic: slots the first pass left to the deep pass, box tests made.  Asking for it adds
 *                               one atomic add per wave.
 *   6. A row is also invalid when t_from[b] is NaN, or when a control point of item 1 of its first n segments is NaN or larger
 *      than 1e300 in magnitude (a non-finite coefficient always gives one; below that bound no halving can overflow).
 *      Invalid rows: status = -1, verdict = DIRECT_PLAN_CHECK_INVALID, t_free = 0, -1 in first, hit_box and seg_first; other
 *      rows are unaffected.
 * CONSERVATIVE BY CONSTRUCTION: a curve lies in the convex hull of its control points, so an unblocked leaf proves its piece of
 * the curve clear.  A blocked verdict means that a piece of the curve of duration T_i / 2^D has a bounding box that touches an
 * occupied voxel (or leaves the map); it does NOT mean that the curve enters that voxel.  A larger depth shrinks the boxes.
 * The result is that of judging all 2^D leaves of every segment one by one; the kernels find it by descending the halving tree
 * and skipping every subtree whose own box is unblocked or that ends at or before t_from (DESIGN.md 6.12 has the argument).
 * DIRECT_ERR_INVALID, nothing launched: a NULL handle / struct / n_seg / T / status; a non-positive batch / n_seg_max; not
 * exactly one of bez and poly; an unknown mem or dtype; depth outside [0, 12]; a non-finite map_lower; margin < 0 or not
 * finite; resolution <= 0 or not finite; outside_blocks not 0 or 1; a handle without a map.  DIRECT_ERR_UNSUPPORTED: batch *
 * n_seg_max of 2^31 or more.  Runs on the handle's stream and synchronises before it returns; direct_cluster_last_ms covers its
 * kernels (not the copies of host arrays).  Its workspace (8 B per row and 16 B per segment slot) and the staging of host
 * arrays grow on demand and are freed in direct_cluster_destroy.  It leaves resident clusters and the path workspace alone. */
#define DIRECT_PLAN_CHECK_INVALID (-1)
typedef struct {
  int32_t batch, n_seg_max;
  int32_t mem;               /* direct_mem_t: where every array of `in` and `out` lives (out->stats: always host) */
  int32_t dtype;             /* direct_dtype_t: storage type of T, bez, poly */
  const int32_t* n_seg;      /* [batch] */
  const void* T;             /* [batch][n_seg_max] */
  const void* bez;           /* [batch][n_seg_max][18] or NULL } exactly one */
  const void* poly;          /* [batch][n_seg_max][18] or NULL }            */
  double map_lower[3];
  double resolution;
  double margin;             /* >= 0 metres added to every box on each side; 0: the map is already inflated */
  int32_t depth;             /* D in [0, 12] */
  int32_t outside_blocks;    /* 0 / 1 */
  const double* t_from;      /* [batch] or NULL */
} direct_plan_check_in_t;

typedef struct {
  int32_t* status;           /* [batch], required */
  int32_t* verdict;          /* [batch] or NULL */
  double* t_free;            /* [batch] or NULL */
  int32_t* first;            /* [batch][2] or NULL */
  int32_t* hit_box;          /* [batch][6] or NULL */
  int32_t* seg_first;        /* [batch][n_seg_max] or NULL */
  int64_t* stats;            /* HOST [2] or NULL */
} direct_plan_check_out_t;

direct_status_t direct_cluster_plan_check_batch(direct_cluster_handle_t h, const direct_plan_check_in_t* in,
                                                direct_plan_check_out_t* out);

/* ---- distance field of the resident map (no reference counterpart) --------------------------------------------------
 * The exact squared Euclidean distance field of the map the handle holds NOW.  For every voxel v of the map,
 *   D2[v] = min over voxels u with byte 1 of (vx-ux)^2 + (vy-uy)^2 + (vz-uz)^2,
 * an int32 in voxel units with the map's own layout (x * max_y * max_z + y * max_z + z).  An occupied voxel has D2 = 0; a map
 * with no occupied voxel has D2 = +infinity everywhere; outside the map there is nothing, so no border convention enters.  The
 * STORED value is min(D2, cap2), cap2 = cap_vox * cap_vox for cap_vox > 0 and DIRECT_DIST_NONE for cap_vox == 0: a stored cap2
 * means "at least this far".  With cap_vox == 0 the field is exact everywhere and DIRECT_DIST_NONE appears only on an empty map.
 * Dimensions are at most 1024 per axis, so every finite D2 is below 2^22 and no sum overflows; an infinite source is skipped,
 * never added to.  All integer work: the result is a pure function of the map, whatever the launch shape.
 * The field is resident on the handle (two buffers of 4 B per voxel, allocated by the first call, freed in
 * direct_cluster_destroy) and VALID from a successful build until the next direct_cluster_set_map or
 * direct_cluster_map_from_cloud call, which mark it stale whether or not they succeed.  direct_cluster_get_distance_field and
 * direct_cluster_plan_clearance_batch return DIRECT_ERR_INVALID with nothing launched when the field is absent or stale: they
 * never rebuild silently, the caller decides when to pay for a rebuild.
 * stats (HOST, [2], or NULL): [0] the number of voxels with a stored value below cap2, [1] the largest stored value below cap2,
 * or -1 if there is none.  Asking for it adds one atomic add and one atomic max per wave of the last pass, on counters of their
 * own.
 * DIRECT_ERR_INVALID, nothing launched: a NULL handle; cap_vox < 0 or above 1024; an unknown mem; a NULL d2; a handle without a
 * map.  Both calls run on the handle's stream and synchronise before they return; the build runs between the handle's event
 * pair, so direct_cluster_last_ms covers it.  They leave resident clusters, the path workspace and the plan-check workspace
 * alone. */
#define DIRECT_DIST_NONE 0x7fffffff
direct_status_t direct_cluster_distance_field(direct_cluster_handle_t h, int32_t cap_vox, int64_t* stats /* HOST [2] or NULL */);
/* The stored field, d2[max_x][max_y][max_z] int32 in memory kind `mem` */
direct_status_t direct_cluster_get_distance_field(direct_cluster_handle_t h, int32_t mem, int32_t* d2);

/* ---- metric clearance of plans (no reference counterpart) --------------------------------------------------------------
 * For each solved plan a certified lower bound on its distance to the occupied voxels, in metres, from the resident distance
 * field; where and when that bound is attained; and from when on the plan is closer than `radius`.  One map then serves any
 * vehicle radius, and candidate plans can be ranked by the air around them.
 * The inputs are those of direct_plan_check_in_t minus margin and outside_blocks, plus radius (finite, >= 0 metres; 0: only the
 * bound is wanted).  Rows and their validity, control points (item 1 of the plan-check block), leaves and their time spans
 * (item 2), "a leaf is judged iff its end time is > t_from[b]" (item 4) and the invalid rows of item 6 are EXACTLY the plan
 * check's.  All arithmetic is double with contraction off, written with plain *, +, - and sqrt.  inv = 1.0 / resolution is
 * computed once on the host.  For one leaf with six points L_j, per axis a:
 *   lo_a = min_j L_j[a], hi_a = max_j L_j[a], c_a = (lo_a + hi_a) * 0.5, e_a = (hi_a - lo_a) * 0.5
 *   half = sqrt((e_0*e_0 + e_1*e_1) + e_2*e_2)
 *   q_a = (c_a - map_lower[a]) * inv; i_a = size_a - 1 when q_a >= size_a, 0 when !(q_a >= 1), else (int)q_a - compared
 *         before it is converted
 *   m_a = ((double)i_a + 0.5) * resolution + map_lower[a], r_a = c_a - m_a
 *   off = sqrt((r_0*r_0 + r_1*r_1) + r_2*r_2)
 * and with d2 the stored field value at (i_0, i_1, i_2):
 *   bound = +inf when d2 == DIRECT_DIST_NONE, else ((sqrt((double)d2) - K) * resolution - off) - half,
 * K = 0x1.bb67ae8584cabp-1 (0.8660254037844387), the smallest double not below sqrt(3)/2.
 * WHY IT IS A LOWER BOUND: the nearest occupied voxel CENTRE is resolution * sqrt(d2) from the voxel centre m; an occupied cube
 * reaches at most sqrt(3)/2 * resolution from its centre; the distance to a set is 1-Lipschitz, c is `off` from m, and every
 * point of the leaf's piece of curve lies in the box of its control points, hence within `half` of c.  A box centre outside the
 * map goes through the same formula with the clamped voxel, `off` carrying the displacement.  A capped field only lowers d2, so
 * the bound stays valid (and cannot exceed about cap_vox * resolution).  Unlike the plan check's verdict this is NOT an exact
 * predicate: it is certified up to the rounding of the fifteen-odd double operations above, about 1e-15 relative.  A negative
 * bound is reported as computed and means "nothing certified".  A larger depth shrinks `half`.
 * Outputs (any but status may be NULL):
 *   status [batch]                 0 or -1 (required)
 *   clearance [batch] (double)     the minimum bound over the judged leaves, in metres; +inf when no leaf is judged or every
 *                                  bound is +inf
 *   where [batch][2]               segment and leaf of that minimum, the first in (segment, leaf) order among equal values;
 *                                  (-1, -1) when there is none (the clearance is +inf)
 *   t_min [batch] (double)         that leaf's start time; S_n when there is none
 *   verdict [batch]                0: every judged bound is >= radius; 1: not; DIRECT_PLAN_CHECK_INVALID for an invalid row
 *   t_free [batch] (double)        the start time of the first judged leaf with bound < radius, in (segment, leaf) order; S_n
 *                                  when the verdict is 0
 *   seg_clearance [batch][n_seg_max] (double)  the minimum per segment (+inf for a segment without a judged leaf).  Entries past
 *                                  n_seg are untouched in device memory and all-ones bytes (a NaN) in host memory.
 * Invalid rows: status = -1, verdict = DIRECT_PLAN_CHECK_INVALID, clearance NaN, t_min = t_free = 0, -1 in where, NaN in the
 * first min(n_seg, n_seg_max) entries of seg_clearance; other rows are unaffected.  The result is that of evaluating all 2^D
 * leaves of every segment one by one; minima are taken with a commutative, associative merge, so it does not depend on the
 * launch shape.
 * DIRECT_ERR_INVALID, nothing launched: as direct_cluster_plan_check_batch (a NULL handle / struct / n_seg / T / status; a
 * non-positive batch / n_seg_max; not exactly one of bez and poly; an unknown mem or dtype; depth outside [0, 12]; a non-finite
 * map_lower; resolution <= 0 or not finite; a handle without a map), plus a radius < 0 or not finite, and a handle without a
 * valid distance field.  DIRECT_ERR_UNSUPPORTED: batch * n_seg_max of 2^31 or more.  Runs on the handle's stream and
 * synchronises before it returns; direct_cluster_last_ms covers its kernels (not the copies of host arrays).  Its workspace
 * (8 B per row and 24 B per segment slot) and the staging of host arrays are blocks of its own on the handle, grown on demand
 * and freed in direct_cluster_destroy.  It leaves resident clusters, the path workspace and the plan-check workspace alone. */
typedef struct {
  int32_t batch, n_seg_max;
  int32_t mem;               /* direct_mem_t: where every array of `in` and `out` lives */
  int32_t dtype;             /* direct_dtype_t: storage type of T, bez, poly */
  const int32_t* n_seg;      /* [batch] */
  const void* T;             /* [batch][n_seg_max] */
  const void* bez;           /* [batch][n_seg_max][18] or NULL } exactly one */
  const void* poly;          /* [batch][n_seg_max][18] or NULL }            */
  double map_lower[3];
  double resolution;
  double radius;             /* >= 0 metres; 0: only the bound is wanted */
  int32_t depth;             /* D in [0, 12] */
  int32_t reserved;
  const double* t_from;      /* [batch] or NULL */
} direct_plan_clear_in_t;

typedef struct {
  int32_t* status;           /* [batch], required */
  double* clearance;         /* [batch] or NULL */
  int32_t* where;            /* [batch][2] or NULL */
  double* t_min;             /* [batch] or NULL */
  int32_t* verdict;          /* [batch] or NULL */
  double* t_free;            /* [batch] or NULL */
  double* seg_clearance;     /* [batch][n_seg_max] or NULL */
} direct_plan_clear_out_t;

direct_status_t direct_cluster_plan_clearance_batch(direct_cluster_handle_t h, const direct_plan_clear_in_t* in,
                                                    direct_plan_clear_out_t* out);

/* ---- cube corridors: the corridors of a batch of grid paths in one call (grid path -> corridor -> optimiser) ------------
 * The corridor of the reference with is_cluster_on == false: paramSet then sets (itr_inflate_max, itr_cluster_max) = (1000, 0)
 * (cluster_server_cpu.cpp:91-97) and every polytope is the inflated cube of its seed voxel alone, six planes - a pure function
 * of the seed voxel and the map.  The cubes of all path points are therefore computed at once, the walk of
 * polyhedronGenerator::corridorGeneration / corridorInsertGeneration (poly_utils.cpp:391-449, 508-557) reduces to a selection,
 * and the planes are written in the layout direct_ddp_batch_in_t reads (planes, n_planes, seeds: pass them on with T0 == NULL).
 * It stands beside the lock-step walk over direct_cluster_polygon_generation_batch(seed, itr_inflate_max, 0) +
 * direct_cluster_hull_planes_batch and gives, bit for bit, that walk's corridors; it does not reproduce corridors of
 * is_cluster_on == true, and it has none of that path's capacities (cluster_capacity, the hull's caps): it succeeds where
 * that path reports an overflow.
 *   Cube     cubeInflation_cpu (cluster_server_cpu.cpp:257-293): from the single voxel, up to itr_inflate_max rounds over the
 *            directions Y-, Y+, X-, X+, Z-, Z+; a face moves out by one voxel when it is not on the map's border and the slab
 *            one voxel beyond it, with the ranges the cube has at that moment, is free; the first round that changes nothing
 *            is the last.  The seed's own byte is not looked at.  The slab test is one query of the handle's summed-area
 *            table, which counts map bytes == 1 where the reference tests > 0: THE CALL IS DEFINED ON THE TABLE and equals the
 *            reference's cube (vertex_idx of direct_cluster_polygon_generation_batch) for maps whose bytes are 0 or 1, which is
 *            all direct_cluster_map_from_cloud produces; direct_cluster_set_map does not validate its bytes.
 *   Planes   what direct_cluster_hull_planes_batch returns for the cube's resident cluster, computed by the same code: the six
 *            lattice planes in ascending (nx, ny, nz, K) order, the half-voxel inflation, the corners of the voxels instead of
 *            their centres when the cube is one voxel thick along an axis, and the centre as the mean over the planes of the
 *            first corner on each (NOT the middle of the box).  n_planes is 6.
 *   Walk     for point i of a row, cur = index * resolution + 0.5 * resolution + map_lower per axis (index2Coord).  A point
 *            equal to the one visited before it is skipped.  With pop_back (corridorGeneration) a point inside the last-but-one
 *            polytope removes the last one.  A point for which the corridor is empty, or with
 *            cur[0]*a + cur[1]*b + cur[2]*c + d > 0.01 for a plane of the latest polytope (isOutsidePolytope; in double, left to
 *            right, no contraction, on the double planes), appends the cube of its own voxel with seed_coord = cur.  Below a
 *            resolution of 0.02 that margin admits a voxel centre one voxel outside the cube, as in the reference.  pop_back == 0
 *            is corridorInsertGeneration started from an empty corridor (extending an existing corridor is not offered).
 * path_xyz[batch][path_capacity][3] int32 and path_len[batch] in memory kind mem_in are exactly the outputs of
 * direct_cluster_grid_path_batch, whose device arrays can be passed through.  batch is NOT limited by max_batch.  Outputs in
 * memory kind `mem`, any may be NULL; planes, seeds and centers are double or float as plane_dtype says (float: one rounding of
 * the double):
 *   n_seg[batch]                          polytopes of the corridor (the number NEEDED, also on overflow)
 *   n_planes[batch][seg_capacity]         6
 *   planes[batch][seg_capacity][p_max][4] p_max >= 6 is the stride of the optimiser's plane array; rows 6 .. p_max - 1 are zero
 *   seeds[batch][seg_capacity][3], centers[batch][seg_capacity][3]
 *   cube_idx[batch][seg_capacity][6]      lo x, y, z, hi x, y, z of every polytope's cube (inclusive voxel indices)
 *   rtn[batch]                            codes below, per row: a failing row does not affect the others
 * Every entry from a row's n_seg on is zero, n_planes included.  No output depends on the launch shape.
 * DIRECT_ERR_INVALID, nothing launched: a handle without a map; a NULL handle, struct, path_xyz or path_len; a non-positive
 * batch, path_capacity, seg_capacity or itr_inflate_max; p_max < 6; an unknown mem_in, mem or plane_dtype; a resolution that is
 * not finite and positive; a non-finite map_lower.  DIRECT_ERR_UNSUPPORTED: batch * path_capacity or batch * seg_capacity *
 * p_max of 2^28 or more.  Runs on the handle's stream and synchronises before it returns; direct_cluster_last_ms covers its
 * two kernels (not the copies of host arrays).  The call follows the map the handle holds now.  Its workspace (28 B per path
 * slot) and the staging of host arrays are blocks of its own on the handle, grown on demand, never shrunk and freed in
 * direct_cluster_destroy; it leaves resident clusters, the grid-path workspace and the distance field alone. */
#define DIRECT_CUBE_CORRIDOR_OK 0
#define DIRECT_CUBE_CORRIDOR_OVERFLOW 1 /* more polytopes than seg_capacity: n_seg is the number needed, the first seg_capacity are valid */
#define DIRECT_CUBE_CORRIDOR_BAD_PATH 2 /* path_len <= 0, path_len > path_capacity (an OVERFLOW row of the path stage), or a voxel outside the map: n_seg 0 */
typedef struct {
  int32_t batch, path_capacity;
  int32_t mem_in;            /* direct_mem_t of path_xyz and path_len */
  int32_t itr_inflate_max;   /* > 0; paramSet's value without clustering is 1000 */
  const int32_t* path_xyz;   /* [batch][path_capacity][3] */
  const int32_t* path_len;   /* [batch] */
  int32_t pop_back;          /* 1: corridorGeneration's walk, 0: corridorInsertGeneration's from an empty corridor */
  int32_t seg_capacity;
  int32_t p_max;             /* >= 6 */
  int32_t plane_dtype;       /* direct_dtype_t of planes, seeds, centers */
  double resolution;
  double map_lower[3];
} direct_cube_corridor_in_t;

typedef struct {
  int32_t mem;               /* direct_mem_t: where every array below lives */
  int32_t reserved;
  int32_t* n_seg;            /* [batch] or NULL */
  int32_t* n_planes;         /* [batch][seg_capacity] or NULL */
  void* planes;              /* [batch][seg_capacity][p_max][4] or NULL */
  void* seeds;               /* [batch][seg_capacity][3] or NULL */
  void* centers;             /* [batch][seg_capacity][3] or NULL */
  int32_t* cube_idx;         /* [batch][seg_capacity][6] or NULL */
  int32_t* rtn;              /* [batch] or NULL */
} direct_cube_corridor_out_t;

direct_status_t direct_cluster_cube_corridor_batch(direct_cluster_handle_t h, const direct_cube_corridor_in_t* in,
                                                   direct_cube_corridor_out_t* out);

/* ---- radius-aware cube corridors: the corridor stage on the resident distance field (no reference counterpart) -----------
 * direct_cluster_cube_corridor_batch with ONE change: a cube stops growing at voxels that are closer to an obstacle than a
 * floor, not only at occupied ones.  It honours the floor of direct_cluster_grid_path_clear_batch / _fan_batch in the same
 * units and with the same refusals, so that path, corridor and direct_cluster_plan_clearance_batch agree on one radius on one
 * map.  Let D2[v] be the STORED field value of voxel v (direct_cluster_distance_field), in voxel^2 units; a voxel is BELOW THE
 * FLOOR when D2[v] < min_d2.  D2 is 0 exactly on bytes == 1, so occupied voxels are below every floor >= 1.
 *   Cube     the plain call's, with obstacles(box) = the number of voxels of the box below the floor.  Round order, border
 *            rule, stop rule and itr_inflate_max are unchanged.  The seed voxel's own D2 is never looked at (as the start's D2
 *            in the path calls): a vehicle closer to a wall than the floor still gets a polytope to start in.
 *   Planes, centre, walk, output layouts and the per-row codes DIRECT_CUBE_CORRIDOR_* are the plain call's; both structs are
 *            reused unchanged.
 *   Neutral  min_d2 <= 1 uses the map's own table and returns the plain call's bytes.  No distance field is needed, and a
 *            stale or missing one is not looked at (the neutral rule of the path calls).
 *   Clear    min_d2 >= 2 reads a FLOOR TABLE: the summed-area table of "below the floor", in the layout of the map's table.
 *            The handle keeps two of them, keyed by (min_d2, the field they were built from): a call whose key is resident
 *            builds nothing, any other call builds into the slot used least recently, so two vehicle sizes alternating on one
 *            map never rebuild.  Every successful direct_cluster_distance_field makes the resident tables stale.
 * Equivalence: the result is, bit for bit, the plain call's on the map whose byte is (D2 < min_d2) ? 1 : 0.
 * WHAT IT GUARANTEES (a derivation, not a measurement; the counterpart of plan_clearance's K).  Every voxel of every cube other
 * than its seed voxel has stored D2 >= min_d2.  A polytope is contained in the union of its cube's voxel cubes (the half-voxel
 * inflation of the planes; the voxels' corners when the cube is degenerate).  A point of a voxel is at most sqrt(3)/2 voxels
 * from its centre, and an occupied voxel cube reaches at most sqrt(3)/2 voxels from its centre.  So every point of a polytope
 * whose seed voxel also satisfies the floor is at least (sqrt(min_d2) - sqrt(3)) * resolution from every occupied voxel cube.
 * On a field built with a cap, stored values at cap2 mean "at least cap2" and the floor may not exceed it.
 * info (HOST, [2] or NULL): info[0] = 1 if this call built a table, 0 if it reused one or ran in neutral mode; info[1] = the
 * number of voxels the table in use counts (neutral mode: the occupied voxels).
 * DIRECT_ERR_INVALID, nothing launched: everything the plain call refuses; min_d2 < 0; and for min_d2 >= 2 a handle whose
 * distance field is missing or older than its map (never a silent rebuild), or min_d2 above the cap2 the field was built with.
 * DIRECT_ERR_UNSUPPORTED as the plain call.  Runs on the handle's stream and synchronises before it returns;
 * direct_cluster_last_ms covers the table build, when there is one, and the two kernels.  The two tables (the size of the
 * map's table each) are allocated together by the first clear-mode call, not by direct_cluster_create, and freed in
 * direct_cluster_destroy.  The call leaves the map and its table, the field, resident clusters and every other workspace alone;
 * it shares the plain call's workspace and staging blocks. */
direct_status_t direct_cluster_cube_corridor_clear_batch(direct_cluster_handle_t h, const direct_cube_corridor_in_t* in, int32_t min_d2,
                                                         direct_cube_corridor_out_t* out, int64_t* info /* HOST [2] or NULL */);

/* ---- clearance-aware grid paths: the path stage on the resident distance field (no reference counterpart) ------------
 * direct_cluster_grid_path_batch with two additions read from the distance field the handle holds: a hard floor ("never
 * closer than this") and a soft cost ("prefer open space, pay for proximity").  Optimal paths on a voxel graph hug corners
 * and walls; this call is the one stage that can give a plan air before the corridor is built.  Let D2[v] be the STORED
 * field value of voxel v (direct_cluster_distance_field), in voxel^2 units.
 *   Graph   the 26 neighbours.  A move goes INTO a voxel v inside the map with map byte 0 AND D2[v] >= min_d2.  D2 is 0
 *           exactly on occupied voxels, so for min_d2 <= 1 this is the graph of direct_cluster_grid_path_batch.  The start
 *           voxel's byte, D2 and penalty are never looked at, as there.
 *   Cost    pen(v) = penalty[D2[v]] if D2[v] < n_penalty, else 0.0.  d(start) = 0 and
 *             d(v) = fl( min over the neighbours u of fl(d(u) + w(u, v)) + pen(v) ),
 *           w the three constants of the plain call: TWO rounded double additions per move, in this order, the step weight
 *           first, then the penalty of the voxel entered.  pen(v) does not depend on u and a -> fl(a + p) is monotone, so
 *           this equals min_u fl(fl(d(u) + w) + pen(v)): the minimum may be taken before the second addition, and that is
 *           the form the kernel uses.  path_cost = d(goal) is the left-to-right fold (((0 + w_1) + pen_1) + w_2) + pen_2 ...
 *           along the emitted path, to the bit.
 *   Path    read backwards from the goal: the predecessor of v is the first neighbour u, in the ascending (dx, dy, dz)
 *           order of the plain call, with fl(fl(d(u) + w) + pen(v)) == d(v) as doubles.
 * One result, whatever the launch shape.  Every value the relaxation holds is the fold of some walk from the start, hence an
 * upper bound of d.  The map a -> fl(fl(a + w) + p) is monotone and >= a because w > 0 and p >= 0; so a heap Dijkstra with
 * these two additions settles voxels in non-decreasing order of d, and by induction along that order the tiled relaxation,
 * whatever order its tiles run in and whichever of a neighbour's old or new values it reads, ends on the same field.
 * Costs never fall along a walk, so a voxel whose value exceeds the goal's current value cannot lie on an optimal path to
 * the goal: pruning by that value stays valid.  d falls STRICTLY along the read-back because w >= 1, so the trace ends.
 * Inputs: batch, starts, goals (HOST, [batch][3]), path_capacity, max_rounds and mem are those of
 * direct_cluster_grid_path_batch; min_d2 >= 0; penalty a HOST array of n_penalty doubles, each finite and >= 0,
 * 0 <= n_penalty <= 65536, NULL only with n_penalty == 0.
 * Outputs in memory kind `mem`, any may be NULL: path_xyz, path_len, path_cost, dist, stats and rtn with the layouts, the
 * exactness contract and the DIRECT_GRID_PATH_* codes of the plain call (NO_PATH also covers a goal with D2 < min_d2 that is
 * not the start), and
 *   path_d2[batch][path_capacity]  the stored D2 of each emitted path voxel (the start's included),
 *   path_min_d2[batch]             the minimum of D2 over ALL voxels of the path except the start - the whole path also on
 *                                  OVERFLOW, as path_len; DIRECT_DIST_NONE for a path of length 1 and where there is no path.
 * DIRECT_ERR_INVALID, nothing launched: what the plain call refuses; a NULL struct; min_d2 < 0; n_penalty outside
 * [0, 65536]; a NULL penalty with n_penalty > 0; a penalty entry that is NaN, infinite or negative; a handle without a map
 * or without a VALID distance field (a stale field is refused as direct_cluster_plan_clearance_batch refuses it, never
 * rebuilt silently); and, on a field built with cap_vox > 0 (cap2 = cap_vox^2), min_d2 > cap2 or n_penalty > cap2: a stored
 * cap2 means "at least cap2", and the call never gives that value two meanings.
 * The call reuses the plain call's workspace (allocated by whichever of the two comes first) and adds the table on the
 * device (512 KiB) and a second read-back ring.  It leaves the map, the distance field, resident clusters and every other
 * workspace alone; direct_cluster_last_ms covers it, direct_cluster_set_stream is honoured. */
typedef struct {
  int32_t batch, path_capacity;
  int32_t max_rounds;        /* 0: the library's default */
  int32_t mem;               /* direct_mem_t of every output */
  const int32_t* starts;     /* HOST [batch][3] */
  const int32_t* goals;      /* HOST [batch][3] */
  int32_t min_d2;            /* >= 0, voxel^2 */
  int32_t n_penalty;         /* 0 .. 65536 */
  const double* penalty;     /* HOST [n_penalty], or NULL with n_penalty == 0 */
} direct_grid_path_clear_in_t;

typedef struct {
  int32_t* path_xyz;         /* [batch][path_capacity][3] or NULL */
  int32_t* path_len;         /* [batch] or NULL */
  double* path_cost;         /* [batch] or NULL */
  double* dist;              /* [batch][max_x*max_y*max_z] or NULL */
  int32_t* stats;            /* [batch][2] or NULL */
  int32_t* rtn;              /* [batch] or NULL */
  int32_t* path_d2;          /* [batch][path_capacity] or NULL */
  int32_t* path_min_d2;      /* [batch] or NULL */
} direct_grid_path_clear_out_t;

direct_status_t direct_cluster_grid_path_clear_batch(direct_cluster_handle_t h, const direct_grid_path_clear_in_t* in,
                                                     direct_grid_path_clear_out_t* out);

/* ---- shared-start grid paths: one field per source, any number of goals (no reference counterpart) ------------------
 * The batches this project is built for nearly always share an endpoint: one vehicle at one place now, many candidate goals.
 * The field d of the two calls above depends on the START alone (they read the goal only to prune, and the read-back never
 * writes the field), so one relaxation per distinct start serves any number of goals.  This call does that, with the plain
 * cost or the clearance-aware one, and returns per goal THE VERY BYTES the pairwise call returns.
 *   Sources  sources[n_src][3], HOST, 1 <= n_src <= max_batch: a source owns one field slot of the workspace the pairwise
 *            calls use (allocated by whichever path call comes first).
 *   Goals    goals[n_goal][3], HOST, n_goal >= 1 and NOT limited by max_batch; goal_src[n_goal] (HOST) names each goal's
 *            source, NULL means all 0 (then n_src must be 1).  A source may have no goal at all.
 *   Modes    NEUTRAL is min_d2 <= 1 && n_penalty == 0: the graph and the cost of direct_cluster_grid_path_batch, no distance
 *            field needed (a stale or missing one is not looked at); path_d2 and path_min_d2 must then be NULL.  Any other
 *            parameters are CLEAR mode: the graph, the two-addition cost and the predecessor rule of
 *            direct_cluster_grid_path_clear_batch, min_d2 / n_penalty / penalty as there.
 * Definition.  For goal j with s = goal_src[j]: path_xyz[j], path_len[j], path_cost[j], rtn[j] (and, in clear mode, path_d2[j]
 * and path_min_d2[j]) are the bytes the pairwise call - the plain one in neutral mode, the clear one otherwise, with the same
 * path_capacity - returns for the single query (sources[s], goals[j]).  Why: with every goal's optimal path exact in the field
 * (below), the predecessor rule reads only values below d(goal), all exact, and picks the lowest matching neighbour: one path.
 * Per-goal codes, the existing five, each for that goal only except where a whole source is named:
 *   BAD_ENDPOINT  the goal is outside the map, or its source is (a source outside the map computes nothing: ALL its goals);
 *   NO_PATH       as in the pairwise calls, a goal that is occupied or below the floor and is not its source included;
 *   OVERFLOW      the needed length and the valid cost are returned, as there;
 *   ROUND_LIMIT   EVERY goal of a source that is still changing when max_rounds is reached (the one code that may differ
 *                 from the pairwise call's: a source relaxes as far as its WORST goal needs);
 *   a goal equal to its source is OK with length 1 and cost 0, whatever the voxel's byte.
 * Pruning.  bound(s) is the maximum of d_s(goal) over the ELIGIBLE goals of s: inside the map, source inside the map, and
 * either equal to the source or enterable (map byte 0 and, in clear mode, D2 >= min_d2).  A goal known to be NO_PATH before
 * anything runs is not eligible and does not switch pruning off for its group; a source without an eligible goal has bound 0
 * and relaxes nothing.  Costs never fall along a walk, so a voxel above the bound lies on no optimal path to any goal of s.
 * Outputs in memory kind `mem`, any may be NULL: the per-goal arrays above, and per source
 *   dist[n_src][max_x*max_y*max_z]  exact wherever the true distance is <= the largest path_cost among the source's eligible
 *           goals (if one of them is unreachable: the whole connected component of the source); elsewhere any value >= the
 *           true distance, +inf included;
 *   stats[n_src][2]  rounds in which the source had an active tile, tile visits: diagnostic, NOT deterministic.
 * Everything but stats, and dist where it is not exact, is independent of the launch shape, of how the goals are grouped and
 * of their order: one call with all goals, the goals split over several calls and a permuted goal list give identical bytes
 * per goal.
 * DIRECT_ERR_INVALID, nothing launched.  From the arguments alone, checked first: a NULL struct, sources or goals; n_src < 1;
 * n_goal < 1; path_capacity <= 0; max_rounds < 0; a bad mem; min_d2 < 0; the table checks of the clear call; a NULL goal_src
 * with n_src != 1; a goal_src entry outside [0, n_src); path_d2 or path_min_d2 in neutral mode.  From the handle: n_src >
 * max_batch; no map; and in clear mode everything direct_cluster_grid_path_clear_batch refuses - a stale or missing distance
 * field, min_d2 or n_penalty above the cap2 the field was built with.
 * Workspace: the fields, flags and counters of the pairwise calls serve the n_src slots; blocks of this call's own, grown on
 * demand and freed in direct_cluster_destroy, hold the goals, their grouping, the bounds and 4 B x path_capacity x n_goal per
 * read-back ring (one for path_xyz, one for path_d2); host outputs go through one staging block.  It leaves the map, the
 * distance field, resident clusters and every other workspace alone; direct_cluster_last_ms covers it,
 * direct_cluster_set_stream is honoured.
 * OUT OF SCOPE: many starts to one goal.  The cost is a left-to-right fold of rounded additions from the START, and a move
 * pays for the voxel it enters; a field relaxed backwards from a shared goal folds the same terms in the other order, so a
 * reversed fan is not bit-equal to the pairwise call, and none is offered. */
typedef struct {
  int32_t n_src, n_goal, path_capacity;
  int32_t max_rounds;        /* 0: the library's default */
  int32_t mem;               /* direct_mem_t of every output */
  const int32_t* sources;    /* HOST [n_src][3] */
  const int32_t* goals;      /* HOST [n_goal][3] */
  const int32_t* goal_src;   /* HOST [n_goal], index into sources; NULL means all 0 (then n_src must be 1) */
  int32_t min_d2;            /* >= 0, voxel^2 */
  int32_t n_penalty;         /* 0 .. 65536 */
  const double* penalty;     /* HOST [n_penalty], or NULL with n_penalty == 0 */
} direct_grid_path_fan_in_t;

typedef struct {
  int32_t* path_xyz;         /* [n_goal][path_capacity][3] or NULL */
  int32_t* path_len;         /* [n_goal] or NULL */
  double* path_cost;         /* [n_goal] or NULL */
  int32_t* rtn;              /* [n_goal] or NULL, DIRECT_GRID_PATH_* */
  int32_t* path_d2;          /* [n_goal][path_capacity] or NULL; NULL in neutral mode */
  int32_t* path_min_d2;      /* [n_goal] or NULL; NULL in neutral mode */
  double* dist;              /* [n_src][max_x*max_y*max_z] or NULL */
  int32_t* stats;            /* [n_src][2] or NULL */
} direct_grid_path_fan_out_t;

direct_status_t direct_cluster_grid_path_fan_batch(direct_cluster_handle_t h, const direct_grid_path_fan_in_t* in,
                                                   direct_grid_path_fan_out_t* out);

/* ---- free-space components and batched reachability (no reference counterpart) ----------------------------------------
 * Which goals can be reached at all.  A pairwise path query whose goal is enterable but not connected ends with NO_PATH only
 * after its relaxation has flooded the start's whole component, and in the fan one such goal switches pruning off for its
 * group.  Connectivity is a pure function of the map and the floor, and it is undirected, because a move needs only the voxel it
 * enters to be enterable: it is built once, kept resident and goes stale with the map, as the distance field does.
 *   Enterable     enterable(v) = map byte of v == 0 && (min_d2 <= 1 || D2[v] >= min_d2), D2 the STORED distance field: word for
 *                 word the "a move goes INTO" rule of direct_cluster_grid_path_batch (min_d2 <= 1) and
 *                 direct_cluster_grid_path_clear_batch.  min_d2 <= 1 needs no field, and a stale or missing one is not looked
 *                 at.  Penalties play no part, because they are finite.
 *   Label         label[v], int32, in the map's layout (x * max_y * max_z + y * max_z + z): -1 for a voxel that is not enterable,
 *                 otherwise the SMALLEST linear index among the voxels of v's component in the graph "enterable voxels, 26
 *                 neighbours inside the map".  A pure function of map bytes, stored field and min_d2: bit for bit the same
 *                 whatever the launch shape and however often it is rebuilt.
 *   Size          size[v], int32: the number of voxels of v's component for an enterable v, else 0.
 *   Stats         stats[4] (int64, HOST, may be NULL): enterable voxels, number of components, size of the largest component, its
 *                 label (-1 without one; ties go to the smaller label).
 *   Reachability  of a pair (s, g), with the codes of the path calls (DIRECT_GRID_PATH_*):
 *                   BAD_ENDPOINT  if s or g lies outside the map;
 *                   OK            if s == g, whatever the voxel's byte;
 *                   NO_PATH       if g is not enterable;
 *                   if s is enterable: OK iff label[s] == label[g];
 *                   if s is NOT enterable: OK iff some 26-neighbour n of s inside the map is enterable and has
 *                                 label[n] == label[g] (the path calls never look at the start's byte, D2 or penalty);
 *                   NO_PATH       otherwise.
 *                 This is exactly the rtn of the pairwise and fan calls with OVERFLOW folded into OK.  ROUND_LIMIT cannot be
 *                 foretold: a query that would run out of max_rounds is judged as if it had not.
 * direct_cluster_free_components builds labels and sizes for the map the handle holds NOW, into one resident pair of int32
 * buffers per handle (4 B per voxel each, allocated by the first build, never shrunk, freed in direct_cluster_destroy).  It runs
 * on the handle's stream and synchronises before it returns; direct_cluster_last_ms covers its kernels.  DIRECT_ERR_INVALID,
 * nothing launched: a NULL handle or no map; min_d2 < 0; min_d2 > 1 without a VALID distance field, or with min_d2 above the
 * cap2 the field was built with (the refusals of the clear path call, with the same wording).  Method: a union-find by smaller
 * index, per 8^3 tile in LDS, then across tile borders in global memory, then a flatten; all integer, every loop bounded - a
 * bound that is passed is DIRECT_ERR_DEVICE, never a hang.
 * direct_cluster_get_free_components fetches label and size ([max_x*max_y*max_z] int32 each) into memory kind `mem` and the
 * normal form of the floor the set was built with (<= 1 -> 0) into *min_d2_built (HOST); any of the three may be NULL.
 * direct_cluster_reachable_batch judges n pairs: n > 0 and NOT limited by max_batch; starts[n][3] and goals[n][3] in memory
 * kind mem_in (a device-resident goal list passes through); outputs in memory kind `mem`, any may be NULL: rtn[n],
 * goal_label[n], goal_size[n] - goal_label is -1 and goal_size is 0 where the goal is outside the map or not enterable.  It
 * does no relaxation: one lane per pair, up to 26 label loads for a start that is not enterable.  DIRECT_ERR_INVALID, nothing
 * launched: a NULL handle, struct, starts or goals; n <= 0; a bad mem / mem_in; min_d2 < 0; no VALID labels; an in->min_d2 whose
 * normal form differs from the one the labels were built with - a label set never gets two meanings.  Host arrays go through
 * staging blocks of the call's own, grown on demand and freed in direct_cluster_destroy.
 * STALENESS.  Labels are marked stale by direct_cluster_set_map and direct_cluster_map_from_cloud, whether or not they succeed;
 * labels built with min_d2 > 1 also by every direct_cluster_distance_field call.  A stale set is refused by the fetch and by
 * direct_cluster_reachable_batch, never rebuilt silently.  The build leaves the map, the field, resident clusters, the floor
 * tables and every path workspace alone. */
direct_status_t direct_cluster_free_components(direct_cluster_handle_t h, int32_t min_d2, int64_t* stats /* HOST [4] or NULL */);
direct_status_t direct_cluster_get_free_components(direct_cluster_handle_t h, int32_t mem, int32_t* label, int32_t* size,
                                                   int32_t* min_d2_built /* HOST or NULL */);
typedef struct {
  int64_t n;                 /* pairs, > 0; not limited by max_batch */
  int32_t mem_in;            /* direct_mem_t of starts and goals */
  int32_t min_d2;            /* >= 0; its normal form must be the one the labels were built with */
  const int32_t* starts;     /* [n][3] */
  const int32_t* goals;      /* [n][3] */
} direct_reachable_in_t;

typedef struct {
  int32_t mem;               /* direct_mem_t: where every array below lives */
  int32_t reserved;
  int32_t* rtn;              /* [n] or NULL, DIRECT_GRID_PATH_OK / _NO_PATH / _BAD_ENDPOINT */
  int32_t* goal_label;       /* [n] or NULL */
  int32_t* goal_size;        /* [n] or NULL */
} direct_reachable_out_t;

direct_status_t direct_cluster_reachable_batch(direct_cluster_handle_t h, const direct_reachable_in_t* in,
                                               direct_reachable_out_t* out);

/* ---- cluster corridors: the corridors of a batch of grid paths with is_cluster_on == true, the walk on the device ---------
 * The cluster-mode twin of direct_cluster_cube_corridor_batch: the corridor the reference ships (inflate, cluster, hull), for many
 * grid paths at once, written in the layout direct_ddp_batch_in_t reads (planes, n_planes, seeds: pass them on with T0 == NULL).
 * It replaces the lock-step walk on the host (polyhedronGenerator::walk of direct_amd/host/poly_utils.hpp), which pays one host
 * round trip per polytope of the longest corridor and reads every plane back to test the next point against it.
 *   Result   per row, bit for bit what that walk produces (poly_utils.cpp:508-557 / :391-449), with getConvexPoly(seed) =
 *            direct_cluster_polygon_generation_batch(seed, itr_inflate_max, itr_cluster_max) + direct_cluster_hull_planes_batch on
 *            the resident cluster with a plane capacity of p_max.  A point is handled in this order: cur = index * resolution +
 *            0.5 * resolution + map_lower per axis (index2Coord); a point equal to the one visited before it is skipped; with
 *            pop_back a point that is not outside the last-but-one polytope removes the last one; a new polytope is due when the
 *            corridor is empty or cur[0]*a + cur[1]*b + cur[2]*c + d > 0.01 for a plane of the latest polytope (double, left to
 *            right, no contraction).  The plane tests always read the DOUBLE planes, never a float output.
 *   Rounds   a row walks on the device until a polytope is due; the seeds due in a round are de-duplicated by voxel (a polytope
 *            is a function of its seed voxel and the map alone; the owner of a voxel is the smallest row that asks for it), the
 *            unique seeds are generated in chunks of at most max_batch, and every waiting row copies its polytope onto its own
 *            plane stack.  No plane, cluster voxel or path point crosses to the host.  What does cross, and stays: one 32-byte
 *            read-back per round (the number of unique seeds decides the chunks), and the generation's own liveness read-back,
 *            one per four clustering rounds of every chunk.
 *   The result does not depend on max_batch, on the order of the rows, on how the rows are split over calls or on the
 *   de-duplication.
 * batch is NOT limited by max_batch.  path_capacity, mem_in, path_xyz[batch][path_capacity][3] and path_len[batch] are exactly
 * the outputs of the three grid-path calls, whose device arrays can be passed through.  itr_inflate_max > 0; itr_cluster_max >= 0,
 * 0 means cubes (then the planes are those of direct_cluster_cube_corridor_batch wherever no capacity of this path is reached).
 * pop_back: 1 corridorGeneration's walk, 0 corridorInsertGeneration's from an empty corridor (extending an existing corridor is
 * not offered).  seg_capacity, p_max (>= 6), plane_dtype, resolution and map_lower as in the cube call.
 * Outputs in memory kind out->mem, any may be NULL; planes, seeds and centers are double or float as plane_dtype says (float: one
 * rounding of the double):
 *   n_seg[batch]                          polytopes of the corridor the row returns (at most seg_capacity)
 *   n_planes[batch][seg_capacity]
 *   planes[batch][seg_capacity][p_max][4] plane rows from a polytope's n_planes on are zero
 *   seeds[batch][seg_capacity][3], centers[batch][seg_capacity][3]
 *   rtn[batch]                            codes below, per row: a failing row never affects another
 * Every entry from a row's n_seg on is zero, n_planes included.
 * stats (HOST, [4] or NULL), all deterministic: [0] rounds in which a seed was due (the rounds of the lock-step walk), [1] due
 * seeds summed over the rounds, [2] unique seeds actually generated, [3] pops.
 * DIRECT_ERR_INVALID, nothing launched: what the cube call refuses (a handle without a map; a NULL handle, struct, path_xyz or
 * path_len; a non-positive batch, path_capacity, seg_capacity or itr_inflate_max; p_max < 6; an unknown mem_in, mem or
 * plane_dtype; a resolution that is not finite and positive; a non-finite map_lower) and a negative itr_cluster_max.
 * DIRECT_ERR_UNSUPPORTED: batch * path_capacity or batch * seg_capacity * p_max of 2^28 or more.  DIRECT_ERR_DEVICE: a device
 * error, or rows still walking after path_capacity + 1 rounds (every unfinished row ends or consumes a point per round, so this
 * bound cannot be reached; it is checked, never spun on).
 * STATE.  The call uses the handle's cluster storage: it INVALIDATES resident clusters, as direct_cluster_convex_test does (a
 * following direct_cluster_hull_planes_batch with cluster_xyz == NULL fails until the next generation).  It leaves the map and
 * its table, the grid-path workspace, the distance field, the floor tables and the free components alone.  It runs on the
 * handle's stream and synchronises before it returns.  direct_cluster_last_ms covers the call from its first kernel to its last,
 * which INCLUDES the waits of its small read-backs (not the copies of host arrays).  Its workspace (64 B per row, the double
 * plane stack of 32 B x batch x seg_capacity x p_max with 52 B per polytope slot beside it, 4 B per voxel for the owner table,
 * the hull outputs of one chunk) and the staging of host arrays are blocks of its own on the handle, grown on demand, never
 * shrunk and freed in direct_cluster_destroy. */
#define DIRECT_CORRIDOR_OK 0
#define DIRECT_CORRIDOR_OVERFLOW 1         /* the walk needed polytope seg_capacity + 1 and stopped there: n_seg = seg_capacity, and those polytopes are the stack at that moment - later points could have popped some of them, so they need not be a prefix of the full corridor */
#define DIRECT_CORRIDOR_BAD_PATH 2         /* path_len <= 0, path_len > path_capacity (an OVERFLOW row of the path stage), or a voxel outside the map: n_seg 0 */
#define DIRECT_CORRIDOR_NO_POLYTOPE 3      /* the generation of a due seed did not end DIRECT_CLUSTER_OK or its hull did not end DIRECT_HULL_OK (the reference's cdd-error branch): the walk stops, n_seg is the polytopes held so far, as walk() leaves them */
#define DIRECT_CORRIDOR_TOO_MANY_PLANES 4  /* a polytope has more than p_max facets: the walk stops in the same way */
typedef struct {
  int32_t batch, path_capacity;
  int32_t mem_in;            /* direct_mem_t of path_xyz and path_len */
  int32_t itr_inflate_max;   /* > 0; paramSet's value is 1000 */
  const int32_t* path_xyz;   /* [batch][path_capacity][3] */
  const int32_t* path_len;   /* [batch] */
  int32_t itr_cluster_max;   /* >= 0; 0: cubes */
  int32_t pop_back;          /* 1: corridorGeneration's walk, 0: corridorInsertGeneration's from an empty corridor */
  int32_t seg_capacity;
  int32_t p_max;             /* >= 6 */
  int32_t plane_dtype;       /* direct_dtype_t of planes, seeds, centers */
  int32_t reserved;
  double resolution;
  double map_lower[3];
} direct_cluster_corridor_in_t;

typedef struct {
  int32_t mem;               /* direct_mem_t: where every array below lives */
  int32_t reserved;
  int32_t* n_seg;            /* [batch] or NULL */
  int32_t* n_planes;         /* [batch][seg_capacity] or NULL */
  void* planes;              /* [batch][seg_capacity][p_max][4] or NULL */
  void* seeds;               /* [batch][seg_capacity][3] or NULL */
  void* centers;             /* [batch][seg_capacity][3] or NULL */
  int32_t* rtn;              /* [batch] or NULL */
} direct_cluster_corridor_out_t;

direct_status_t direct_cluster_corridor_batch(direct_cluster_handle_t h, const direct_cluster_corridor_in_t* in,
                                              direct_cluster_corridor_out_t* out, int64_t* stats /* HOST [4] or NULL */);

/* The HIP stream (hipStream_t) the handle enqueues its copies, kernels and timing events on; NULL (the default) is
 * the legacy default stream.  Mirrors direct_ddp_set_stream. */
direct_status_t direct_cluster_set_stream(direct_cluster_handle_t h, void* hip_stream);
/* HIP-event time [ms] of the kernels of the last polygon_generation_batch / convex_test / hull_planes_batch /
 * grid_path_batch / map_from_cloud / plan_check_batch / distance_field / plan_clearance_batch / cube_corridor_batch /
 * grid_path_clear_batch / grid_path_fan_batch / free_components / reachable_batch / corridor_batch / map_integrate_scan /
 * frontier call (the fan: its init,
 * bounds, rounds, read-back and stats kernels with the read-backs of the round counters between them, not the copies of host
 * arrays; the components: the two clears and the four kernels of a build, the one kernel of reachable_batch; corridor_batch:
 * from its first kernel to its last, the waits of its read-backs included) */
direct_status_t direct_cluster_last_ms(direct_cluster_handle_t h, float* ms);

/* ---- one sensor scan folded into the map: carve the free space, mark the returns ------------------------------------
 * direct_cluster_map_from_cloud can forget everything (REPLACE) or never forget anything (ADD).  This call uses the other half
 * of a range measurement: the ray from the sensor to a return is empty.  A spurious return, a door that has opened or a person
 * who has walked on leaves the map with the next scan that looks through the place.  There is no reference counterpart (the
 * reference builds its map once); the definition below is this library's own and is restated by tests/map_scan_harness.py.
 * The handle keeps a second resident grid, the SCAN GRID `raw`: the map's size and layout, bytes 0 or 1, allocated by the
 * first call.  One call is one scan, four steps in order:
 *   1. Carve    every ray from `origin` to a point writes 0 into the raw voxels it passes (the walk below).
 *   2. Mark     every HIT ray writes 1 into the raw voxel of its point.  All carving precedes all marking, and each phase
 *               writes one byte value only: the result depends neither on the order of the points nor on the launch shape, and
 *               the returns of this scan always survive it.
 *   3. Inflate  map[x,y,z] = 1 exactly when some raw voxel with |dx| <= inflate[0], |dy| <= inflate[1], |dz| <= inflate[2]
 *               INSIDE the map is 1: a voxel box, no wrap; inflate = {0,0,0} makes the map equal raw.  This is deliberately NOT
 *               the coordinate inflation of direct_cluster_map_from_cloud: dilating raw is what lets a carved voxel take its
 *               shell with it.  Callers of the radius-aware calls (min_d2, radius) pass zeros; callers of
 *               direct_cluster_corridor_batch, which has no floor, pass their radius in voxels.
 *   4. Tables   while the map is written, the voxels that change 0 -> 1 and 1 -> 0 are counted against the bytes the map held
 *               before the call, whoever wrote them.  If anything changed, or the handle had no map, the call has
 *               direct_cluster_set_map's effect on everything the handle holds (the summed-area table is rebuilt by the same
 *               code; the distance field, the floor tables and the free components are stale; resident clusters stay).  If
 *               NOTHING changed, all of them stay valid and nothing is rebuilt: a node that scans a static room at 10 Hz pays
 *               for no field.  Rebuild the field when stats[6] + stats[7] > 0.
 * Unknown space does not enter the MAP: a voxel never seen is free there, as in the reference (what has been seen is recorded
 * beside it on request: "known space and frontier goals" below).  THIS call counts no hits and keeps no log-odds: the last
 * observation wins.  Evidence per voxel lives in a call of its own, direct_cluster_map_integrate_scan_evidence ("occupancy
 * evidence per voxel" below), which derives the scan grid and the map from a resident evidence grid; a plain scan past its
 * refusals writes the scan grid behind that grid's back and therefore drops it.
 * The walk.  All in double, no square root; inv = 1.0 / resolution and R2 = max_range * max_range computed once on the host;
 * e_a = (double)p_a, d_a = e_a - origin_a, dd = (d_x*d_x + d_y*d_y) + d_z*d_z without fused multiply-adds.  A ray is a HIT when
 * dd <= R2, otherwise TRUNCATED: it carves out to max_range and marks nothing.  Start voxel i: the origin's, by the DROP rule of
 * direct_cluster_map_from_cloud.  End voxel of a hit: j_a = (int)floor((e_a - map_lower_a) * inv), inside when 0 <= j_a < size_a
 * for all a.  Per axis step_a = sign(d_a), n_a = |j_a - i_a| for a hit, and for step_a != 0: b = map_lower_a + (double)(i_a +
 * (step_a > 0)) * resolution, tmax_a = (b - origin_a) / d_a, tdel_a = resolution / fabs(d_a).  Loop: stop without writing when
 * the current voxel is outside the map; a hit stops when n_x + n_y + n_z steps are done; choose the axis with the smallest tmax
 * among those with step != 0 and, for a hit, n_a > 0 (ties: the lower axis); clear the current voxel; a truncated ray stops here
 * when !((t*t)*dd <= R2) for the chosen t = tmax_a; then i_a += step_a, tmax_a += tdel_a, n_a -= 1.  A hit clears every voxel
 * before j and ends in j exactly, by counting; a truncated ray clears its last voxel too.  A point with a non-finite coordinate
 * contributes nothing.
 * xyz[n_points][stride] floats in memory kind `mem`.  stats (host [8], may be NULL): [0] points read, [1] points skipped as
 * non-finite, [2] truncated rays, [3] hits whose voxel lies outside the map (no mark), [4] raw voxels at 1 after the call,
 * [5] map voxels at 1 after the call, [6] map voxels that went 0 -> 1, [7] map voxels that went 1 -> 0.
 * DIRECT_ERR_INVALID (the handle is left as it was): null handle or parameters; n_points < 0; xyz == NULL with n_points > 0; an
 * unknown mem, mode or stride; a resolution or max_range that is not finite and positive; a non-finite map_lower or map_upper;
 * an origin outside [map_lower, map_upper) or beyond the last voxel; a negative inflate; ADOPT without a map.
 * DIRECT_ERR_UNSUPPORTED: max_range * inv above 4096; an inflate above 64.  n_points == 0 is legal: RESET then gives an empty map.
 * After DIRECT_ERR_DEVICE the handle has neither a map nor a scan grid.
 * Runs on the handle's stream and synchronises before it returns; direct_cluster_last_ms covers the clears, the kernels, the
 * wait for the counters and the table (not the copy of a host cloud).  The scan grid (1 B per voxel) lives as long as the
 * handle; the two intermediate grids of an inflation in y or z are a block of their own, grown on demand. */
#define DIRECT_SCAN_RESET    0  /* the scan grid starts empty */
#define DIRECT_SCAN_CONTINUE 1  /* keep it; a handle without one starts empty */
#define DIRECT_SCAN_ADOPT    2  /* the scan grid starts as the bytes of the map the handle holds (INVALID without a map) */
#define DIRECT_SCAN_TRACK_KNOWN 1  /* direct_map_scan_t.flags bit 0: record what this scan observed in the known grid (below) */
typedef struct {
  double map_lower[3], map_upper[3];
  double resolution, max_range;
  double origin[3];
  int32_t inflate[3];
  int32_t mode, stride /* 3 or 4 */, flags /* DIRECT_SCAN_TRACK_KNOWN or 0; any other bit: DIRECT_ERR_INVALID, "unknown flags" */;
} direct_map_scan_t;
direct_status_t direct_cluster_map_integrate_scan(direct_cluster_handle_t h, const direct_map_scan_t* p, int64_t n_points,
                                                  int32_t mem, const float* xyz, int64_t* stats /* host [8] or NULL */);
/* The scan grid, raw[max_x*max_y*max_z] in memory kind `mem`; DIRECT_ERR_INVALID before the first scan. */
direct_status_t direct_cluster_get_scan_grid(direct_cluster_handle_t h, int32_t mem, uint8_t* raw);
/* For measurements: ms4[0..3] = HIP-event time [ms] of the carve, the mark, the inflation and the table rebuild (0 when nothing
 * changed) of the last scan.  Recorded only by a handle created with DIRECT_CLUSTER_SCAN_TIMING=1 in the environment
 * (DIRECT_ERR_INVALID otherwise); DIRECT_CLUSTER_SCAN_STORE=plain makes the carve store without loading the byte first. */
direct_status_t direct_cluster_scan_phase_ms(direct_cluster_handle_t h, float* ms4);

/* ---- known space and frontier goals ----------------------------------------------------------------------------------
 * The KNOWN GRID is a third resident grid: the map's size and layout, one byte per voxel, 1 = observed, 0 = never observed.  It is
 * allocated by the first call that needs it.  A scan with DIRECT_SCAN_TRACK_KNOWN in direct_map_scan_t.flags fills it from the
 * walk it does anyway: every voxel the carve clears and every voxel the mark sets also gets known = 1 (a hit outside the map marks
 * nothing).  Every writer writes 1, in both phases: the known grid depends neither on the order of the points nor on the launch
 * shape.  With the flag, RESET empties the known grid too, CONTINUE and ADOPT keep it (a handle without one starts empty; ADOPT
 * says nothing about what was seen - a caller with prior knowledge uses direct_cluster_set_known).  The scan grid, the map and
 * the stats of a tracked scan are those of the same scan untracked.  A scan with flags == 0 is the call it has always been, and
 * on a handle that holds a known grid it DROPS the grid: its rays were not recorded.  A tracked scan that fails on the device
 * leaves no known grid.  direct_cluster_set_map and direct_cluster_map_from_cloud leave the known grid alone: it describes
 * observation, not occupancy.
 * direct_cluster_get_known: known[max_x*max_y*max_z] in memory kind `mem`; DIRECT_ERR_INVALID when the handle holds no known grid.
 * direct_cluster_set_known: the handle's known grid becomes (known[v] != 0) of the caller's bytes, or all zero for known == NULL -
 * a persisted grid, a declared-known box around the take-off point, a prior map.  It synchronises before it returns.
 *
 * direct_cluster_frontier turns map + known grid into a short ordered list of goal voxels, all integer and exact:
 *   frontier voxel  known != 0, and enterable as the path calls see it (map byte 0 and, for min_d2 > 1, stored D2 >= min_d2: every
 *                   frontier voxel is a legal goal of direct_cluster_grid_path_fan_batch under the same floor), and at least one of
 *                   its 6 face neighbours INSIDE the map has known == 0.  The outside of the map is not unknown space.
 *   component       a 26-connected component of the frontier voxels, labelled by its smallest linear index.
 *   kept            size >= min_size.  The kept components in ascending label order fill the outputs; the first `capacity` are
 *                   written.  stats[3] > capacity: call again with more room.
 *   centroid        c_a = (2 * sum_a + n) / (2 * n) per axis (int64): the rounded mean of the members' coordinates.  It may be
 *                   occupied, unknown or outside the component.
 *   rep             the goal: the member that minimises (min(dist2, 0xffffffff) << 32) | linear index, dist2 = sum (v_a - c_a)^2:
 *                   nearest the centroid voxel, ties to the smaller index.  Always known, enterable and on the frontier.
 * stats: [0] known voxels, [1] frontier voxels, [2] components, [3] kept components, [4] written = min(kept, capacity), [5] the
 * size of the largest component.  Entries of the per-component arrays from stats[4] on: -1 in host memory, untouched in device
 * memory.  Any output may be NULL; capacity == 0 is a count-only call.
 * DIRECT_ERR_INVALID, nothing launched, in this order: NULL handle, in or out; an unknown mem; min_d2 < 0, min_size < 1 or
 * capacity < 0; capacity > 0 with label, size, centroid and rep all NULL; no map; no known grid; for min_d2 > 1, no valid distance
 * field or min_d2 above its cap.  DIRECT_ERR_DEVICE: a device error, or the labelling's error word.
 * The labelling is the union-find of direct_cluster_free_components on a mask grid, with buffers of this call's own: the
 * resident free components are not touched and stay valid.  The call changes nothing else the handle holds, runs on the handle's
 * stream and synchronises before it returns; direct_cluster_last_ms covers its clears and kernels.  Its workspace (13 B per voxel
 * and 44 B per slot) and the staging of host outputs are blocks of its own on the handle, grown on demand, never shrunk and
 * freed in direct_cluster_destroy; a handle that never calls it allocates nothing. */
typedef struct { int32_t min_d2, min_size, capacity, mem; } direct_frontier_in_t;
typedef struct {
  int32_t* label;        /* [capacity]     smallest linear index of the component */
  int32_t* size;         /* [capacity]     its voxel count */
  int32_t* centroid;     /* [capacity][3]  rounded centroid voxel (may be occupied or unknown) */
  int32_t* rep;          /* [capacity][3]  the goal: a voxel OF the component nearest the centroid voxel */
  int32_t* voxel_label;  /* [G] or NULL    per voxel: its frontier component's label, -1 elsewhere */
  int64_t* stats;        /* HOST [6] or NULL */
} direct_frontier_out_t;
direct_status_t direct_cluster_get_known(direct_cluster_handle_t h, int32_t mem, uint8_t* known);
direct_status_t direct_cluster_set_known(direct_cluster_handle_t h, int32_t mem, const uint8_t* known /* or NULL: all zero */);
direct_status_t direct_cluster_frontier(direct_cluster_handle_t h, const direct_frontier_in_t* in, const direct_frontier_out_t* out);
/* For measurements: ms4[0..3] = HIP-event time [ms] of the mask, the labelling, the compaction and the goals (sums,
 * representatives, unpack) of the last frontier call, recorded as direct_cluster_scan_phase_ms records (DIRECT_CLUSTER_SCAN_TIMING=1). */
direct_status_t direct_cluster_frontier_phase_ms(direct_cluster_handle_t h, float* ms4);

/* ---- occupancy evidence per voxel: scans that count hits and misses ---------------------------------------------------
 * direct_cluster_map_integrate_scan lets the last observation win: one spurious return occupies a voxel, one grazing ray erases a
 * thin obstacle.  This call accumulates instead, in the manner of clamped log-odds with one update per voxel and scan, in
 * integers: the result is exactly defined and depends neither on the order of the points nor on the launch shape.  It is restated
 * by tests/evidence_harness.py.  There is no reference counterpart.
 * The EVIDENCE GRID is a further resident grid: the map's size and layout, one int8 per voxel, 0 = no information, allocated by
 * the first call that needs it.  `scan` (geometry, inflate, mode, stride, flags) is read exactly as the plain call reads it.
 * One call is one scan, five steps in order on the handle's stream:
 *   0. Start    RESET: ev = 0 everywhere (with DIRECT_SCAN_TRACK_KNOWN the known grid is emptied too, as in the plain call).
 *               CONTINUE: keep ev; a handle without an evidence grid starts from zeros.  ADOPT: ev[v] = (map[v] == 1) ? ev_max : 0
 *               (DIRECT_ERR_INVALID without a map, as in the plain call).
 *   1. Touch    a per-call touch grid starts at 0; every ray writes 1 into exactly the voxels the plain scan's carve would clear
 *               (the same walk).
 *   2. Hit      every HIT ray whose voxel is inside the map writes 2 into the touch byte of that voxel.  All of step 1 precedes
 *               all of step 2 and each phase writes one value: a voxel both passed and hit in one scan is a hit.
 *   3. Fold     once per voxel, in int arithmetic with t = touch[v] and e = ev[v]:  t == 2: e = min(e + hit, ev_max);
 *               t == 1: e = max(e - miss, ev_min);  t == 0: e is unchanged, even where it lies outside this call's clamp (an
 *               earlier call with other limits, or set_evidence, may have left it there).  Then ev[v] = e and
 *               raw[v] = (e >= occ) for EVERY voxel, touched or not: behind every evidence scan the scan grid is a function of
 *               the evidence grid and occ alone, and whatever a plain scan left in it is overwritten.  With
 *               DIRECT_SCAN_TRACK_KNOWN known[v] |= (t != 0); with flags == 0 a known grid the handle holds is dropped, as the
 *               plain call drops it.
 *   4. Inflate and tables: steps 3 and 4 of the plain call, on the same code - raw dilated into the map, 0 -> 1 and 1 -> 0
 *               counted against the bytes the map held, the table rebuilt and the field, floor tables and components stale ONLY
 *               if something changed or the handle had no map.
 * n_points == 0 is legal; with CONTINUE it re-thresholds: after set_evidence, or with another occ, it derives scan grid and map
 * from the evidence alone.
 * stats (host [12], may be NULL): [0..7] as in the plain call; [8] voxels touched as hit, [9] voxels touched as pass only,
 * [10] voxels with ev > 0 after the call, [11] voxels with ev < 0 after the call.
 * Refused, the handle left as it was: first everything the plain call refuses, in its order and by its messages (the
 * DIRECT_ERR_UNSUPPORTED ones included); then DIRECT_ERR_INVALID for hit, miss, ev_min, ev_max, occ, reserved, in this order, each
 * by a message that names the field.  After DIRECT_ERR_DEVICE the handle has no map, no scan grid and no evidence grid, and a
 * tracked scan leaves no known grid.
 * direct_cluster_set_map and direct_cluster_map_from_cloud leave the evidence grid alone (it describes observation: the next
 * CONTINUE evidence scan derives the map again and counts its changes against the bytes it finds); direct_cluster_frontier and
 * direct_cluster_view_gain_batch do not touch it.
 * direct_cluster_get_evidence: ev[max_x*max_y*max_z] in memory kind `mem`; DIRECT_ERR_INVALID when the handle holds no evidence grid.
 * direct_cluster_set_evidence: the evidence grid becomes max(ev[v], -127) of the caller's bytes, or all zero for ev == NULL.  It
 * synchronises before it returns and touches neither the map nor the scan grid: they follow at the next evidence scan.
 * direct_cluster_evidence_phase_ms: ms5[0..4] = HIP-event time [ms] of the touch, the hit, the fold, the inflation and the table
 * rebuild (0 when nothing changed) of the last evidence scan, recorded as direct_cluster_scan_phase_ms records. */
typedef struct {
  direct_map_scan_t scan;   /* geometry, inflate, mode, stride, flags: exactly as for direct_cluster_map_integrate_scan */
  int32_t hit, miss;        /* added for a return / subtracted for a pass, 1 .. 127 each */
  int32_t ev_min, ev_max;   /* clamp of a TOUCHED voxel: -127 <= ev_min <= 0, occ <= ev_max <= 127 */
  int32_t occ;              /* a voxel is occupied when ev >= occ; 1 <= occ <= ev_max */
  int32_t reserved[3];      /* must be 0 */
} direct_map_evidence_t;    /* 112 + 32 = 144 bytes */
direct_status_t direct_cluster_map_integrate_scan_evidence(direct_cluster_handle_t h, const direct_map_evidence_t* p, int64_t n_points,
                                                           int32_t mem, const float* xyz, int64_t* stats /* host [12] or NULL */);
direct_status_t direct_cluster_get_evidence(direct_cluster_handle_t h, int32_t mem, int8_t* ev);
direct_status_t direct_cluster_set_evidence(direct_cluster_handle_t h, int32_t mem, const int8_t* ev /* or NULL: all zero */);
direct_status_t direct_cluster_evidence_phase_ms(direct_cluster_handle_t h, float* ms5);

/* ---- visible unknown volume per candidate viewpoint --------------------------------------------------------------------
 * direct_cluster_view_gain_batch says which goal is worth flying to: for every candidate voxel v0 (direct_frontier_out_t.rep, say)
 * it casts the rays of a direction set from the centre of v0 through the resident map and counts, all integer and exact,
 *   seen     the DISTINCT voxels the rays pass,
 *   gain     those of them with known == 0: the growth of the known grid if an ideal sensor with these rays scanned the map as it
 *            stands from the centre of v0,
 *   ends[4]  the rays by outcome: [0] blocked, [1] left the map, [2] out of range, [3] skipped.
 * THE WALK of a direction dir (three floats, map frame, any length), in voxel units, double, no square root: d_a = (double)dir_a,
 * dd = (d_x*d_x + d_y*d_y) + d_z*d_z, R2 = range_vox * range_vox.  The ray is SKIPPED when a component is not finite or dd == 0.
 * step_a = sign(d_a); for step_a != 0, tdel_a = 1.0 / fabs(d_a) and tmax_a = 0.5 * tdel_a; i = v0.  Then, in this order: i outside
 * the map ends the ray LEFT (i is not visited); i is visited; a map byte != 0 at i ends it BLOCKED (the voxel an ideal return would
 * mark); c is the axis with the smallest tmax among those with step != 0, ties to the lower axis; t = tmax_c, and
 * !((t*t)*dd <= R2) ends it out of RANGE; else i_c += step_c, tmax_c += tdel_c.  This is the carve walk of a truncated ray of
 * direct_cluster_map_integrate_scan from a voxel centre, stopped at the first occupied voxel.  No offset from v0 exceeds
 * floor(range_vox + 0.5) per axis.
 * DIRECTION SETS: dirs holds n_sets sets of n_dirs directions, set[c] says which one candidate c uses (NULL: set 0) - several
 * headings of a sensor with a limited field of view in one call, with no trigonometry on the device.
 * code[c]: DIRECT_VIEW_OK; DIRECT_VIEW_OUTSIDE, the voxel is outside the map; DIRECT_VIEW_OCCUPIED, its map byte is != 0;
 * DIRECT_VIEW_BAD_SET, set[c] is outside [0, n_sets) - checked in this order.  A candidate that is not OK gets zeros in gain, seen
 * and ends and casts no ray.
 * Refused, nothing launched and nothing written, in this order: a NULL handle, in or io; an unknown mem_in or mem; n < 0,
 * n_dirs < 1, n_sets < 1; a range_vox that is not finite or <= 0; with n > 0, a NULL voxel or dirs, or code, gain, seen and ends
 * all NULL (DIRECT_ERR_INVALID); floor(range_vox) + 2 > 50 or n_dirs > 65536 (DIRECT_ERR_UNSUPPORTED: the candidate's box of
 * (2R+1)^3 bits, R = floor(range_vox) + 2, lives in LDS); no map; no known grid (DIRECT_ERR_INVALID).  n == 0 past these checks is
 * DIRECT_OK.  DIRECT_ERR_DEVICE: a device error, or the kernel's error word (a walk outside its box or past its trip bound).
 * The call reads the map and the known grid and changes nothing the handle holds.  voxel, set and dirs are read from memory kind
 * mem_in, the outputs written to memory kind mem; device arrays are used in place.  It runs on the handle's stream and
 * synchronises before it returns; direct_cluster_last_ms covers its kernel.  Its staging blocks are the handle's own, grown on
 * demand, never shrunk and freed in direct_cluster_destroy.  For measurements: DIRECT_CLUSTER_VIEW_THREADS = 256, 512 or 1024 in
 * the environment of direct_cluster_create sets the threads per workgroup (1024 otherwise; no output depends on it). */
#define DIRECT_VIEW_OK 0
#define DIRECT_VIEW_OUTSIDE 1
#define DIRECT_VIEW_OCCUPIED 2
#define DIRECT_VIEW_BAD_SET 3
typedef struct { double range_vox; int32_t n, n_dirs, n_sets, mem_in, mem; } direct_view_gain_in_t;
typedef struct {
  const int32_t* voxel;   /* [n][3], e.g. direct_frontier_out_t.rep */
  const int32_t* set;     /* [n] or NULL (all 0): which direction set each candidate uses */
  const float*   dirs;    /* [n_sets][n_dirs][3], map frame, any length */
  int32_t *code, *gain, *seen, *ends;   /* [n], [n], [n], [n][4]; any may be NULL, not all */
} direct_view_gain_io_t;
direct_status_t direct_cluster_view_gain_batch(direct_cluster_handle_t h, const direct_view_gain_in_t* in,
                                               const direct_view_gain_io_t* io);

/* ---- unknown space as occupied: a closed planning map kept by the scans -----------------------------------------------
 * Every planning call reads the map, and the map byte of a voxel nobody has observed is 0: paths, corridors, plan_check, the
 * distance field and the free components take unobserved space for free.  The UNKNOWN POLICY of a handle says what the scans make
 * of it.  DIRECT_UNKNOWN_FREE (the default, and what an all-zero handle means) is the behaviour described so far, kernel for
 * kernel.  Under DIRECT_UNKNOWN_OCCUPIED every scan - direct_cluster_map_integrate_scan and ..._scan_evidence alike - derives TWO
 * grids, all integer and exact; `raw` is the scan grid behind this scan's carve/mark or fold, `known` the known grid behind it:
 *   open[v] = dilate(raw, inflate)[v]      the OPEN MAP: what the scan produces under DIRECT_UNKNOWN_FREE, byte for byte
 *   map[v]  = open[v] | (known[v] == 0)    the MAP: unobserved voxels are closed.  Unknown space is NOT inflated.
 * A known voxel is occupied in the map exactly when it is occupied in the open map, so the known, enterable voxels are the same
 * under both policies, direct_cluster_frontier with min_d2 == 0 returns the same outputs, and every frontier representative stays a
 * legal path goal.  Every planning call reads the map and is safe with no change of its own; direct_cluster_view_gain_batch reads
 * the open map where the handle holds one (its rays must pass unknown voxels to count them) and the map otherwise.
 * stats of a scan under the policy: [4] the ones of raw as before; [5] the ones of the MAP, [6] / [7] the voxels of the MAP set /
 * cleared against the bytes the map held before.  The summed-area table is rebuilt, and the field, the floor tables and the labels
 * go stale, only if the handle had no map or set + cleared > 0: a repeated scan that teaches nothing costs its kernels alone.
 * The result depends neither on the order of the points nor on the launch shape.
 * Under the policy a scan WITHOUT DIRECT_SCAN_TRACK_KNOWN is refused with DIRECT_ERR_INVALID, behind every other refusal of the
 * call and before any write (an untracked scan drops the known grid; nothing would say what is known).  DIRECT_SCAN_ADOPT adopts
 * the OPEN MAP where the handle holds one and the map otherwise - the plain scan's copy and the evidence fold's map operand:
 * adopting the closed map would turn unknown space into returns.
 * The open map is one more byte per voxel, allocated by the first scan under the policy.  The handle HOLDS an open map from a
 * successful scan under the policy until the next scan past its refusals (a successful one under the policy leaves a new one; one
 * under DIRECT_UNKNOWN_FREE, or a device error, leaves none) or the next direct_cluster_set_map / direct_cluster_map_from_cloud
 * past its null check: those two write the caller's bytes verbatim under either policy.  direct_cluster_set_known changes only the
 * known grid; the map follows at the next scan (a CONTINUE tracked scan of no points derives it at once).  It is the way to seed a
 * known bubble around a vehicle whose sensor does not see its own surroundings.
 * direct_cluster_set_unknown_policy: DIRECT_ERR_INVALID for a NULL handle or any other value, nothing written.  It touches no grid
 * and raises no map event: the policy takes effect at the next scan.
 * direct_cluster_get_unknown_policy: *policy, and in stats2 (host, or NULL) [0] closed = voxels with map == 1 and open == 0 and
 * [1] open_ones = the ones of the open map, both of the last successful scan under the policy, zeros when the handle holds no
 * open map.
 * direct_cluster_get_open_map: out[max_x*max_y*max_z] in memory kind `mem`, as direct_cluster_get_map; DIRECT_ERR_INVALID, "the
 * handle has no open map", unless the last writer of the map was a successful scan under DIRECT_UNKNOWN_OCCUPIED.
 * Out of scope: inflating unknown space or a margin from it in metres (direct_cluster_plan_clearance_batch on the closed map
 * reports the distance to the nearest unknown-or-occupied voxel); the outside of the map is not unknown space. */
#define DIRECT_UNKNOWN_FREE     0
#define DIRECT_UNKNOWN_OCCUPIED 1
direct_status_t direct_cluster_set_unknown_policy(direct_cluster_handle_t h, int32_t policy);
direct_status_t direct_cluster_get_unknown_policy(direct_cluster_handle_t h, int32_t* policy, int64_t* stats2 /* host [2] or NULL */);
direct_status_t direct_cluster_get_open_map(direct_cluster_handle_t h, int32_t mem, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* DIRECT_CLUSTER_H_ */
