/*
 * pp_hip.h -- C ABI of the MI355X-native planner core (libpphip.so).
 *
 * Drop-in boundary for the hot path of lfilipozzi/PathPlanning.
 * The reference has no FFI of its own: its plugin surface is the C++ abstract
 * classes StateValidator / PathPlanner plus the pybind11 module.  These entry
 * points are what those classes call into (see INTEGRATION.md for the binding a
 * reference maintainer adds).  Each function cites the reference interface it
 * replaces, paths relative to the reference's planner/src.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (never throws);
 *     pp_last_error() gives the message of the calling thread's last failure;
 *   - *_dev functions take DEVICE pointers and only enqueue work on the context's
 *     stream (no host synchronisation); the others take HOST pointers, copy,
 *     run and synchronise;
 *   - poses are 3 contiguous doubles {x, y, theta} exactly like Pose2d
 *     (geometry/2dplane.h:17-34); grids are row-major, index = row*cols + col,
 *     row <- x, col <- y (utils/grid.h:87, state_validator/occupancy_map.h:106-117);
 *   - no torch types, no C++ types, no global state besides the error string.
 */
#ifndef PP_HIP_H
#define PP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_OK 0
#define PP_ERR_INVALID (-1)
#define PP_ERR_HIP (-2)
#define PP_ERR_NO_DEVICE (-3)
#define PP_ERR_CAPACITY (-4)

typedef struct pp_ctx pp_ctx;         /* one device + one stream */
typedef struct pp_map pp_map;         /* device-resident map set of one OccupancyMap */
typedef struct pp_planner pp_planner; /* Hybrid-A* tables + per-query workspaces */
typedef struct pp_footprint pp_footprint; /* vehicle footprint: discs in the vehicle frame, bound to one map */

const char* pp_last_error(void);
int pp_version(void);

/* ---- context ----------------------------------------------------------- */
/* stream == NULL: the context creates and owns a stream; otherwise it enqueues
 * on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int pp_ctx_create(int device, void* stream, pp_ctx** out);
int pp_ctx_destroy(pp_ctx* ctx);
int pp_ctx_synchronize(pp_ctx* ctx);
/* Non-blocking: *idle = 1 when everything enqueued on the context's stream has completed (hipStreamQuery), else 0.
 * For callers that keep several contexts busy and refill whichever finishes first. */
int pp_ctx_is_idle(pp_ctx* ctx, int32_t* idle);
/* HIP-event timer on the context's stream: start, stop -> milliseconds. */
int pp_ctx_timer_start(pp_ctx* ctx);
int pp_ctx_timer_stop(pp_ctx* ctx, float* ms);
int pp_device_count(void);

/* ---- map set ------------------------------------------------------------
 * Replaces the data members of OccupancyMap (state_validator/occupancy_map.h:122-133),
 * GVD::ObstacleDistanceMap::m_distance (state_validator/gvd.h:58), GVD::PathCostMap
 * (gvd.h:111-121) and the StateSpaceSE2 bounds (state_space/state_space.h:60-61). */
typedef struct pp_map_desc {
	int32_t rows, cols;
	float resolution;         /* OccupancyMap::resolution (float) */
	double grid_origin[2];    /* m_worldGridOrigin */
	double local_origin[2];   /* m_localOrigin */
	double lower[3], upper[3]; /* StateSpaceSE2::bounds */
} pp_map_desc;

int pp_map_create(pp_ctx* ctx, const pp_map_desc* desc, pp_map** out);
int pp_map_destroy(pp_map* map);
/* int32 squared distances to the nearest obstacle, INT_MAX = none (gvd.cpp:21). */
int pp_map_upload_dist2(pp_map* map, const int32_t* d2_host);
/* The same grid as the reference's accessor returns it: float distance in metres,
 * ObstacleDistanceMap::GetDistanceToNearestObstacle(row, col) = sqrt(d2) * resolution (gvd.h:38).  Either upload
 * serves; this one needs no access to the private int grid and loses nothing for INT_MAX / d2 > 2^24 cells. */
int pp_map_upload_distance(pp_map* map, const float* distance_host);
/* int32 occupancy, >= 0 occupied, < 0 free (obstacle_list_occupancy_map.cpp:63-69). */
int pp_map_upload_occupancy(pp_map* map, const int32_t* occ_host);
/* float Voronoi-field potential, GVD::GetPathCost (gvd.h:160-162). */
int pp_map_upload_path_cost(pp_map* map, const float* cost_host);
/* ---- map authoring and field construction on the device ----
 * Shape::RasterizeLine (state_validator/obstacle.cpp:7-61) for n segments given by their world end points (the caller rotates and
 * translates the shape's vertices, PolygonShape::GetVerticesPosition, obstacle.cpp:86-93), writing `value` into every boundary
 * cell: an obstacle id for ObstacleListOccupancyMap::AddObstacle, -1 for RemoveObstacle
 * (obstacle_list_occupancy_map.cpp:29-61).  n_cells_out (may be NULL): cells written, with repeats. */
int pp_map_rasterize_segments(pp_map* map, int32_t n_segments, const double* p0_xy_host, const double* p1_xy_host, int32_t value, int32_t* n_cells_out);
/* The same walk with the cells listed instead of written (Shape::GetGridCellsPosition, Obstacle::GetBoundaryGridCellPosition):
 * segment i fills cells_host[i * cap_per_segment * 2 ...] with (row, col) pairs in Bresenham order, count_host[i] of them.
 * pp_map_set_cells writes `value` into listed cells (AddObstacle / RemoveObstacle for any Shape, also caller-defined ones). */
int pp_rasterize_cells(pp_map* map, int32_t n_segments, const double* p0_xy_host, const double* p1_xy_host, int32_t cap_per_segment, int32_t* cells_host,
	int32_t* count_host);
int pp_map_set_cells(pp_map* map, int64_t n_cells, const int32_t* cells_host, int32_t value);
int pp_map_download_occupancy(pp_map* map, int32_t* occ_host);
/* GVD::Update (state_validator/gvd.cpp:294-301) from the device occupancy grid: squared obstacle distance + nearest obstacle cell
 * (ObstacleDistanceMap::Update, gvd.cpp:30-72), Voronoi edges (CheckVoro, :105-131), squared distance to the nearest edge
 * (VoronoiDistanceMap::Update, :200-237), PathCostMap (:266-283; alpha, d_max: GVD::alpha / dMax, gvd.h:181); also refreshes what
 * the validator reads.  Two modes for the two distance maps:
 *   PP_GVD_REFERENCE_ORDER  the reference's dynamic brushfire itself, replayed (on the host: it is a sequential priority-queue sweep
 *                           whose order among equal keys is part of the result) over the ORDERED cell edits this map has received
 *                           -- pp_map_set_cells / pp_map_rasterize_segments in call order, cells in list order, i.e.
 *                           SetObstacle / UnsetObstacle (gvd.cpp:74-89) as AddObstacle / RemoveObstacle issue them; a
 *                           pp_map_upload_occupancy counts as an empty map followed by its occupied cells in row-major order.
 *                           Grids equal the reference's bit for bit; edits after the first update are incremental.
 *   PP_GVD_EXACT_EDT        exact Euclidean transform on the device (milliseconds, no host round trip): true minima, which the
 *                           brushfire's values are not always, and its own tie rule -- NOT the reference's bits on a few cells in
 *                           ten thousand.  pp_map_update_gvd = this mode.
 * iterations_out (may be NULL): heap pops of the brushfire so far / device passes. */
enum { PP_GVD_EXACT_EDT = 0, PP_GVD_REFERENCE_ORDER = 1 };
int pp_map_update_gvd_ex(pp_map* map, float alpha, float d_max, int32_t mode, int32_t* iterations_out);
int pp_map_update_gvd(pp_map* map, float alpha, float d_max, int32_t* iterations_out);
/* any pointer may be NULL; nearest_*: (row, col) per cell, (-1, -1) = none */
int pp_map_download_gvd(pp_map* map, int32_t* d2_host, int32_t* nearest_obstacle_host, uint8_t* voronoi_edge_host, int32_t* voronoi_d2_host, int32_t* nearest_edge_host,
	float* path_cost_host);
/* PathCostMap::Update alone (gvd.cpp:266-283) over two squared-distance grids of the caller; keeps the result as the map's path
 * cost and copies it out when path_cost_host != NULL. */
int pp_path_cost_update(pp_map* map, const int32_t* obstacle_d2_host, const int32_t* voronoi_d2_host, float alpha, float d_max, float* path_cost_host);

/* StateValidatorOccupancyMap::minSafeRadius / minPathInterpolationDistance
 * (state_validator/state_validator_occupancy_map.h:27-28). */
int pp_map_set_validator(pp_map* map, float min_safe_radius, float min_path_interpolation_distance);
/* Copies the derived float distance grid back (tests): (float)(sqrt((double)d2) * resolution), gvd.h:38. */
int pp_map_download_distance(pp_map* map, float* dist_host);

/* ---- a1: StateValidatorOccupancyMap::IsStateValid -------------------------
 * (state_validator/state_validator_occupancy_map.cpp:15-26), batched. */
int pp_check_states(pp_map* map, int64_t n, const double* poses_host, uint8_t* valid_host);
int pp_check_states_dev(pp_map* map, int64_t n, const double* poses_dev, uint8_t* valid_dev);
/* Fused microbench form ("M1 fused"): poses are generated in-kernel from a
 * counter-based hash, only a per-block count of valid poses leaves the kernel. */
int pp_check_states_fused_dev(pp_map* map, int64_t n, uint64_t seed, uint64_t* valid_count_dev);

/* ---- a2+a3: IsPathValid over constant-steer arcs --------------------------
 * (state_validator_occupancy_map.cpp:28-71 with paths/path_constant_steer.cpp:11-20 and
 * models/kinematic_bicycle_model.cpp:5-32).  curvature = cos(beta)*tan(steer)/wheelbase
 * (kinematic_bicycle_model.cpp:17), computed by the caller with libm. direction: 0 fwd, 1 bwd. */
int pp_check_arcs_dev(pp_map* map, int64_t n, const double* from_dev, const double* curvature_dev, const double* length_dev,
	const int32_t* direction_dev, uint8_t* valid_dev, float* last_ratio_dev);
int pp_check_arcs(pp_map* map, int64_t n, const double* from_host, const double* curvature_host, const double* length_host,
	const int32_t* direction_host, uint8_t* valid_host, float* last_ratio_host);
/* R2 segments (paths/path_r2.cpp) against the same validator with theta = 0: the
 * RRT / RRT* edge check on an occupancy map. */
int pp_check_segments_dev(pp_map* map, int64_t n, const double* from_xy_dev, const double* to_xy_dev, uint8_t* valid_dev);
int pp_check_segments(pp_map* map, int64_t n, const double* from_xy_host, const double* to_xy_host, uint8_t* valid_host);

/* ---- a4: HybridAStar::StatePropagator::GetConstantSteerChild ---------------
 * (algo/hybrid_a_star.cpp:111-147, 41-48, 93-109; hybrid_a_star.h:104-111).
 * One child per (parent, primitive), reference order: primitive p = 2*deltaIndex + dir. */
typedef struct pp_hybrid_params {
	double wheelbase;                /* SearchParameters::wheelbase */
	double min_turning_radius;
	double direction_switching_cost;
	double reverse_cost_multiplier;
	double forward_cost_multiplier;
	double voronoi_cost_multiplier;
	uint32_t num_generated_motion;
	double spatial_resolution;
	double angular_resolution;
	/* reference-behaviour switches; 1 = as the Release build behaves */
	int32_t heading_alias;    /* Q6 */
	int32_t negative_k_read;  /* Q7 */
} pp_hybrid_params;

int pp_rollout_children_dev(pp_map* map, const pp_hybrid_params* params, int32_t n_primitives, const double* curvature_host,
	const int32_t* direction_host, int64_t n_parents, const double* parents_dev, uint8_t* valid_dev, double* pose_dev, int32_t* key_dev,
	double* cost_dev, double* length_dev);
int pp_rollout_children(pp_map* map, const pp_hybrid_params* params, int32_t n_primitives, const double* curvature_host,
	const int32_t* direction_host, int64_t n_parents, const double* parents_host, uint8_t* valid_host, double* pose_host, int32_t* key_host,
	double* cost_host, double* length_host);

/* ---- a6: ReedsShepp::Solver::GetOptimalPath -------------------------------
 * (geometry/reeds_shepp.cpp:654-683), one (from, to) pair per element.
 * word: PathWords index or -1; tuv: the three parameters; cost: float as the
 * reference compares it; seg_length: normalised length. */
int pp_rs_solve_dev(pp_ctx* ctx, int64_t n, const double* from_dev, const double* to_dev, double min_turning_radius, float reverse_cost,
	float forward_cost, float switch_cost, int32_t* word_dev, double* tuv_dev, float* cost_dev, double* seg_length_dev);
int pp_rs_solve(pp_ctx* ctx, int64_t n, const double* from_host, const double* to_host, double min_turning_radius, float reverse_cost,
	float forward_cost, float switch_cost, int32_t* word_host, double* tuv_host, float* cost_host, double* seg_length_host);

/* ---- a7: PathReedsShepp as a value (paths/path_reeds_shepp.{h,cpp}) ---------
 * What the reference's object holds: m_init, m_final, the five ReedsShepp::Motion slots of its PathSegment
 * (geometry/reeds_shepp.h:54-67: steer, direction, normalised length; +inf / NoMotion = unused slot),
 * m_minTurningRadius and m_length (metres; after Truncate it is scaled by the ratio and no longer the sum of the slots).
 * steer: 0 Left, 1 Straight, 2 Right (paths/path.h:10-14); direction: 0 Forward, 1 Backward, 2 NoMotion (:16-20). */
typedef struct pp_rs_path {
	double start[3];
	double final_pose[3];
	double motion_length[5];
	int8_t steer[5];
	int8_t direction[5];
	int8_t reserved[6];
	double min_turning_radius;
	double length;
	float cost;   /* pp_rs_connect: PathSegment::ComputeCost of the chosen word (float, as the reference compares it) */
	int32_t word; /* pp_rs_connect: PathWords index, -1 = NoPath; carried along otherwise */
} pp_rs_path;

/* PathConnectionReedsShepp::Connect (path_reeds_shepp.cpp:174-179): GetOptimalPath + the PathReedsShepp constructor
 * (m_final = Interpolate(1.0)), one path per (from, to) pair. */
int pp_rs_connect(pp_ctx* ctx, int64_t n, const double* from_host, const double* to_host, double min_turning_radius, float reverse_cost,
	float forward_cost, float switch_cost, pp_rs_path* paths_host);
/* PathReedsShepp::Interpolate (:12-47) and ::GetDirection (:155-167) of path i at ratio_host[i]; either output may be NULL. */
int pp_rs_path_interpolate(pp_ctx* ctx, int64_t n, const pp_rs_path* paths_host, const double* ratio_host, double* pose_host, int32_t* direction_host);
/* PathReedsShepp::Truncate (:49-93) in place, INCLUDING the reference's wrong-slot reset when q11 != 0 (SURVEY
 * Appendix A Q11: truncating inside motion i < 4 invalidates motion i itself); q11 == 0 drops the later motions instead. */
int pp_rs_path_truncate(pp_ctx* ctx, int64_t n, pp_rs_path* paths_host, const double* ratio_host, int32_t q11);
/* PathReedsShepp::GetCuspPointRatios (:95-121): ascending, no duplicates; ratios_host is [n][4], count_host[i] <= 4. */
int pp_rs_path_cusps(pp_ctx* ctx, int64_t n, const pp_rs_path* paths_host, double* ratios_host, int32_t* count_host);
/* StateValidatorOccupancyMap::IsPathValid (state_validator_occupancy_map.cpp:28-71) over Reeds-Shepp paths. */
int pp_check_rs_paths_dev(pp_map* map, int64_t n, const pp_rs_path* paths_dev, uint8_t* valid_dev, float* last_ratio_dev);
int pp_check_rs_paths(pp_map* map, int64_t n, const pp_rs_path* paths_host, uint8_t* valid_host, float* last_ratio_host);
/* ... and over PathSE2 (paths/path_se2.cpp:5-22: position and heading interpolated linearly, length = |to - from|). */
int pp_check_se2_paths(pp_map* map, int64_t n, const double* from_host, const double* to_host, uint8_t* valid_host, float* last_ratio_host);

/* ---- vehicle footprint: multi-disc collision test ----------------------------
 * An extension with no counterpart in the reference, whose validator compares ONE look-up of the obstacle-distance grid at
 * the pose's reference point with minSafeRadius.  A footprint is K discs, 1 <= K <= 8, each (ox, oy, r): centre in the
 * vehicle frame (origin = the pose's reference point, x forward, y left; metres) and radius (finite, >= 0).
 * rho = max_i hypot(ox_i, oy_i).
 *
 * State check of a pose (x, y, theta):
 *  1. the reference point passes everything IsStateValid tests except the distance comparison: local position inside the
 *     state bounds, wrapped heading inside the heading bounds, cell inside the grid;
 *  2. for every disc in order: centre cx = (x + ox*c) - oy*s, cy = (y + ox*s) + oy*c with (s, c) = sin, cos of the
 *     UNWRAPPED theta in double (a disc with ox == 0 && oy == 0 uses (x, y) itself and no trigonometry).  The centre must
 *     lie inside the position bounds and its cell (same truncation as the reference point's) inside the grid; then
 *     d_i = distance grid at that cell, and the disc passes iff d_i >= r_i (float compare);
 *  3. valid iff all pass.  clearance = min_i (d_i - r_i) as float; border = (float) min over the reference point and every
 *     disc centre of its four distances to the position bounds (double min, then one conversion).
 * Path check: the march of IsPathValid (state_validator_occupancy_map.cpp:28-71) with
 *     step = fmaxf(fminf(clearance, border) / gain, minPathInterpolationDistance)          (all float)
 *     gain = (float)(1.0 + kappaMax * rho)                                               (double, then one conversion)
 * because a disc centre moves up to (1 + kappa * rho) times as fast as the reference point while the vehicle turns.
 * kappaMax: |curvature| of a constant-steer arc; 1 / min_turning_radius of a Reeds-Shepp path; |to.theta - from.theta| /
 * length of a PathSE2.  last_ratio, the zero-length case and the sample limit are IsPathValid's.  minSafeRadius plays no part
 * once a footprint is used.  The footprint {(0, 0, minSafeRadius)} is the point validator, bit for bit.
 * A footprint follows its map's distance grid: after pp_map_upload_dist2 / pp_map_upload_distance / pp_map_update_gvd* the
 * next check uses the new grid.  A footprint used with another map than its own is PP_ERR_INVALID. */
#define PP_FOOTPRINT_MAX_DISCS 8
typedef struct pp_footprint_disc {
	double ox, oy; /* centre in the vehicle frame, metres */
	float r;       /* radius, metres */
	float pad;
} pp_footprint_disc;
/* n_discs outside 1..8, a non-finite value or a negative radius: PP_ERR_INVALID.  The footprint keeps its map alive. */
int pp_footprint_create(pp_map* map, int32_t n_discs, const pp_footprint_disc* discs, pp_footprint** out);
int pp_footprint_destroy(pp_footprint* fp);
/* Pure host arithmetic, no device: n equal discs on the long axis covering a length x width rectangle whose rear edge lies
 * rear_overhang behind the reference point: s = length / n, ox_i = -rear_overhang + (i + 0.5) * s, oy_i = 0,
 * r = sqrt((s/2)^2 + (width/2)^2) rounded UP to float.  discs_out holds n_discs records. */
int pp_footprint_cover_rectangle(double length, double width, double rear_overhang, int32_t n_discs, pp_footprint_disc* discs_out);
/* The state check above, batched.  clearance_host may be NULL; where the pose is invalid it receives -1. */
int pp_check_states_footprint(pp_map* map, pp_footprint* fp, int64_t n, const double* poses_host, uint8_t* valid_host, float* clearance_host);
int pp_check_states_footprint_dev(pp_map* map, pp_footprint* fp, int64_t n, const double* poses_dev, uint8_t* valid_dev);
/* The path check above over constant-steer arcs (arguments as pp_check_arcs), Reeds-Shepp paths (pp_check_rs_paths) and
 * PathSE2 (pp_check_se2_paths). */
int pp_check_arcs_footprint_dev(pp_map* map, pp_footprint* fp, int64_t n, const double* from_dev, const double* curvature_dev, const double* length_dev,
	const int32_t* direction_dev, uint8_t* valid_dev, float* last_ratio_dev);
int pp_check_arcs_footprint(pp_map* map, pp_footprint* fp, int64_t n, const double* from_host, const double* curvature_host, const double* length_host,
	const int32_t* direction_host, uint8_t* valid_host, float* last_ratio_host);
int pp_check_rs_paths_footprint_dev(pp_map* map, pp_footprint* fp, int64_t n, const pp_rs_path* paths_dev, uint8_t* valid_dev, float* last_ratio_dev);
int pp_check_rs_paths_footprint(pp_map* map, pp_footprint* fp, int64_t n, const pp_rs_path* paths_host, uint8_t* valid_host, float* last_ratio_host);
int pp_check_se2_paths_footprint(pp_map* map, pp_footprint* fp, int64_t n, const double* from_host, const double* to_host, uint8_t* valid_host, float* last_ratio_host);

/* ---- a10: NonHolonomicHeuristic::Build (algo/heuristics.cpp:36-76) ---------
 * dims = {nX, nY, nAngular}; table[(i*nY + j)*nAngular + k]. */
int pp_nonholo_dims(const double lower[3], const double upper[3], const pp_hybrid_params* params, int32_t dims[3], double offsets[2]);
int pp_nonholo_build_dev(pp_ctx* ctx, const double lower[3], const double upper[3], const pp_hybrid_params* params, double* table_dev);
int pp_nonholo_build(pp_ctx* ctx, const double lower[3], const double upper[3], const pp_hybrid_params* params, double* table_host);

/* ---- a8: ObstaclesHeuristic::Update (algo/heuristics.cpp:106-153) ----------
 * One wavefront per goal; cost_dev is [n_goals][rows*cols] float, +inf where the
 * reference leaves the cell unexplored.  The reference's values bit for bit (first discovery,
 * no relaxation, LIFO ties): built as the fixed point those rules define, one wave per goal over
 * 64 x 64-cell tiles (pp_wavefront_tiles.hip); a goal whose value could depend on the pop order among
 * equal costs is detected and rebuilt in the reference's own order (pp_wavefront.hip), as is every goal
 * when PP_WF_TILES=0 is in the environment.  goal_xy: world positions. */
int pp_obstacle_heuristic_dev(pp_map* map, int32_t n_goals, const double* goal_xy_host, float* cost_dev);
int pp_obstacle_heuristic(pp_map* map, int32_t n_goals, const double* goal_xy_host, float* cost_host);
/* ---- heuristic clearance ---------------------------------------------------
 * The validator refuses every pose whose reference point has dist < min_safe_radius; the reference's obstacle heuristic floods over every
 * cell that is merely unoccupied.  A heuristic clearance is a float radius, finite and >= 0.  FOR THE HEURISTIC ONLY a cell is then
 * blocked iff
 *     occupied[cell]  ||  !(dist[cell] >= radius)
 * with the float comparison of the validator (IsStateValid) on the map's distance grid.  Everything else of a8 is untouched: the diagonal
 * rule, the goal cell costing 0 even when blocked, a goal outside the map giving a field of +inf, blocked cells keeping +inf.  radius == 0
 * switches it off: the launch is the one of pp_obstacle_heuristic, same kernels, same arguments.  Validity, costs, the Voronoi term, the
 * non-holonomic table, open list and RNG are never affected.  The field is the reference's field of the map whose occupancy grid has the
 * blocked cells added.
 * Admissibility: with radius <= min_safe_radius the heuristic stays a lower bound wherever the reference's was (no valid pose lies in a
 * cell it blocks); the same holds with a vehicle footprint when radius is at most the radius of a disc that sits on the reference point.
 * A larger radius is the caller's choice and is not refused: the field then overestimates, and may be +inf where a plan exists.
 * The two occupancy views the field kernels read (bytes, padded bit rows) are built from the distance and occupancy grids in one pass on
 * the map's stream, lazily, and rebuilt whenever either grid has been written since.  A map without a distance grid: PP_ERR_INVALID. */
/* pp_obstacle_heuristic[_dev] under the rule above (radius 0: exactly those entries).  Negative or non-finite radius: PP_ERR_INVALID. */
int pp_obstacle_heuristic_clearance_dev(pp_map* map, float radius, int32_t n_goals, const double* goal_xy_host, float* cost_dev);
int pp_obstacle_heuristic_clearance(pp_map* map, float radius, int32_t n_goals, const double* goal_xy_host, float* cost_host);
/* Diagnostics: what building the two occupancy views of a clearance costs on this map -- the mean of `reps` launches of the view kernel
 * into buffers of the call's own, between HIP events on the context's stream, in ms (allocation and a first build are not timed). */
int pp_heuristic_clearance_build_ms(pp_map* map, float radius, int32_t reps, float* ms_out);
/* Diagnostics of the tile form (a stamped instantiation of its kernel): the same fields into cost_dev ([n_goals][rows*cols]), plus 16 words
 * {goals built, tile visits, bucket rounds, candidate passes, cells settled, goals handed to the ordered kernel,
 * summed wave cycles, tiles per goal, then shader-clock sums of a tile visit's phases: loads + LDS set-up, the rounds' masks,
 * their candidate passes, re-queueing, store issue; 3 spare} and the launch's duration in ms (HIP events on the context's stream).
 * handed_over_host (optional, [n_goals]): the indices of the goals that were handed over, in no particular order.
 * PP_ERR_INVALID when the tile form is switched off or does not support the map. */
int pp_obstacle_heuristic_tiles_stats(pp_map* map, int32_t n_goals, const double* goal_xy_host, float* cost_dev, uint64_t stats_host[16], float* ms_out, int32_t* handed_over_host);
/* Diagnostics: stamped build of the wavefront kernel; per goal 20 words {init, min, partition, sort, offer, push,
 * tail cycles, rounds, sum of window sizes, rounds with the open list in HBM, fallback rounds, push cycles of fallback rounds,
 * offer sub-phases: store wait, neighbourhood loads, candidate count, whole offer up to the end of insertion,
 * push sub-phases (cumulative from the start of push): look-up, slot scan, stores; one pad word}. */
int pp_obstacle_heuristic_profile(pp_map* map, int32_t n_goals, const double* goal_xy_host, uint64_t* counters_host);
/* bytes of scratch pp_obstacle_heuristic_dev keeps per concurrently running goal */
int64_t pp_obstacle_heuristic_workspace_bytes(pp_map* map);

/* ---- a5/a9/a11: HybridAStar graph search, batched --------------------------
 * (algo/hybrid_a_star.cpp:59-91,149-173,237-257; algo/a_star.h:326-427;
 * algo/heuristics.cpp:78-95,155-165; utils/frontier.h).  One independent query per
 * (start, goal, seed); seed reseeds the query's own mt19937_64 (utils/random.h). */
int pp_planner_create(pp_map* map, const pp_hybrid_params* params, int32_t max_batch, int32_t max_nodes_per_query, pp_planner** out);
/* Same with an explicit number of search rows.  Planners sized for throughput (max_batch > 64) run the graph search
 * four queries per wave on a persistent grid whose rows take queries from a counter; node / heap / key-map buffers
 * exist per ROW, not per query.  search_rows = 0: as many rows as can be resident on the device (or max_batch if
 * smaller); callers that keep several planners in flight on one GPU pass resident rows / planners. */
int pp_planner_create_ex(pp_map* map, const pp_hybrid_params* params, int32_t max_batch, int32_t max_nodes_per_query, int32_t search_rows,
	pp_planner** out);
/* Diagnostics: the search tree of query q in creation order (parent index, pose, {pathCost, totalCost}, replaced flag);
 * available while node records are kept per query (one-query-per-wave kernel).  Any pointer may be NULL. */
int pp_planner_debug_nodes(pp_planner* planner, int32_t q, int32_t max_nodes, int32_t* parents_host, double* poses_host, double* costs_host,
	int32_t* dead_host);
/* ... and per node the action that created it (-1 root, 0..P-1 constant-steer primitive, 1000 + word Reeds-Shepp) and the
 * length of that edge: with the poses above, the reference's GetGraphSearchExploredPathSet (algo/hybrid_a_star.cpp:186-198). */
int pp_planner_debug_node_actions(pp_planner* planner, int32_t q, int32_t max_nodes, int32_t* action_host, double* length_host);
/* Rows the planner's search runs with (k_hybrid_search_rows); 0 = the one-query-per-wave kernel (k_hybrid_search). */
int pp_planner_search_rows(pp_planner* planner);
int pp_planner_destroy(pp_planner* planner);
/* Uses a table built elsewhere (host pointer), or builds it on the device when NULL. */
int pp_planner_set_nonholo_table(pp_planner* planner, const double* table_host);
int pp_planner_get_nonholo_table(pp_planner* planner, double* table_host);
int pp_planner_num_primitives(pp_planner* planner);
/* Vehicle footprint for the search (see "vehicle footprint" above): everything that asks "is this pose / arc / Reeds-Shepp path valid"
 * -- the start pose, each child's own pose, the arc march and its truncation, the analytic expansion -- goes through the footprint;
 * heuristics, costs, open list, RNG gate and discretisation are untouched.  fp == NULL: back to the point validator.  The planner holds
 * a reference to the footprint.  One-query-per-wave planners only: a planner that runs the rows kernel (pp_planner_search_rows() > 0;
 * create it with max_batch <= 64, or with PP_SEARCH_ROWS=0 in the environment) or is a pipeline's buffer set (a pipeline takes its footprint through
 * pp_pipeline_set_footprint), and a footprint of another map, are PP_ERR_INVALID. */
int pp_planner_set_footprint(pp_planner* planner, pp_footprint* fp);
/* Heuristic clearance of the planner's obstacle heuristic (see "heuristic clearance" above): for the fields of every later
 * pp_planner_search_batch[_dev] a cell is blocked iff occupied[cell] || !(dist[cell] >= radius); the search itself (validity, costs, the
 * other heuristics, open list, RNG) is untouched.  One-query-per-wave and rows planners alike: the field launch is shared.  radius == 0
 * (the default) is the reference's rule.  Each planner keeps occupancy views of its own, so planners with different radii share a map.
 * Waits for the planner's stream.  Negative or non-finite radius: PP_ERR_INVALID; so is a pipeline's buffer set (a pipeline takes its
 * radius through pp_pipeline_set_heuristic_clearance).  radius > min_safe_radius is accepted: see the admissibility note. */
int pp_planner_set_heuristic_clearance(pp_planner* planner, float radius);
int pp_planner_heuristic_clearance(pp_planner* planner, float* radius);
/* Replaces StatePropagator::m_deltas (algo/hybrid_a_star.cpp:21-28 generates {0, +-0.5 dMax, +-1.0 dMax, ...} from num_generated_motion,
 * which can only give 2 * odd primitives): any list of steering angles [rad]; every angle gives a forward and a backward primitive,
 * children in list order, forward first (hybrid_a_star.cpp:65-77).  36 angles = the "72 motion primitives" of BASELINE config 2.
 * Waits for the planner's stream; applies from the next batch on. */
int pp_planner_set_primitives(pp_planner* planner, int32_t n_steering_angles, const double* steering_angles);

typedef struct pp_query_result {
	int32_t status;        /* 0 = Success, -1 = Failure (algo/path_planner.h:9-12), -4 = node capacity exceeded */
	int32_t n_expanded;    /* expansions (frontier pops that were expanded) */
	int32_t n_nodes;       /* nodes created */
	int32_t n_path;        /* poses on the solution path (root..goal) */
	double cost;           /* GetGraphSearchOptimalCost */
	int32_t n_rng_draws;
	int32_t n_rs_attempts;
	int64_t n_state_checks;
	int64_t n_path_checks;
	/* Guard band of the exactness contract: poses of this query (start, children, Reeds-Shepp child) whose
	 * DiscretizePose (hybrid_a_star.h:104-111) truncated a coordinate within 1e-9 cells of a lattice boundary -- the only places
	 * where a last-bit libm difference could select another cell.  0: the query's discrete outputs equal the reference's by
	 * construction; > 0 (e.g. a start or goal placed exactly on a multiple of the resolution): equal as far as observed. */
	int32_t n_lattice_boundary_hits;
	int32_t reserved;
} pp_query_result;

/* Runs the batch (obstacle heuristic + graph search per query).  All pointers host. */
int pp_planner_search_batch(pp_planner* planner, int32_t n_queries, const double* starts_host, const double* goals_host,
	const uint64_t* seeds_host, pp_query_result* results_host);
/* Same, inputs already resident (starts/goals/seeds device pointers); results stay on the device until fetched. */
int pp_planner_search_batch_dev(pp_planner* planner, int32_t n_queries, const double* starts_dev, const double* goals_dev,
	const uint64_t* seeds_dev);
int pp_planner_fetch_results(pp_planner* planner, int32_t n_queries, pp_query_result* results_host);
/* Throughput use, several planners with a batch in flight each (own stream each): the NEXT pp_planner_search_batch*_dev of `planner`
 * starts on the device only when the obstacle-heuristic fields of `predecessor`'s most recently launched batch are built (one-shot,
 * cleared by that call).  Batches launched together otherwise run in phase -- all wavefronts, then all searches, then all tails of long
 * queries with the GPU nearly empty; started one wavefront apart they interleave.  Scheduling only: results do not depend on it. */
int pp_planner_start_after_fields_of(pp_planner* planner, pp_planner* predecessor);
/* Solution path of query q: poses (3*n_path doubles), per-node action kind (0 root, 1 arc, 2 Reeds-Shepp),
 * primitive index (arc) or RS word, arc length; expanded: cells in expansion order (3*n_expanded ints). Any pointer may be NULL. */
int pp_planner_get_path(pp_planner* planner, int32_t q, double* poses_host, int32_t* kind_host, int32_t* prim_host, double* length_host,
	double* tuv_host);
int pp_planner_get_expanded(pp_planner* planner, int32_t q, int32_t* cells_host);
/* Diagnostics: the obstacle-heuristic field the search of query q read ([rows*cols] floats, row-major, +inf where unexplored), as the
 * planner's last batch built it -- the field of pp_obstacle_heuristic (or, with a heuristic clearance, pp_obstacle_heuristic_clearance)
 * for that query's goal.  On pp_pipeline_planner() q is a field slot (pp_pipeline_slot_of of a completed, held ticket). */
int pp_planner_get_obstacle_field(pp_planner* planner, int32_t q, float* cost_host);
/* ---- after the graph search: HybridAStar::SearchPath's post-processing, batched -----------------
 * (algo/hybrid_a_star.cpp:260-304: composite path of the solution's edges, sampling every path_interpolation metres with
 * cusp snapping, then Smoother::Smooth, algo/smoother.cpp:33-226) for the first n_queries queries of the last batch, one
 * workgroup per query.  Needs the nearest-obstacle / nearest-Voronoi-edge cell grids on the map (pp_map_update_gvd builds
 * them, pp_map_upload_nearest_cells takes the reference's GVD::GetNearestObstacleCell / GetNearestVoronoiEdgeCell).
 * smoother == NULL: Smoother::Parameters defaults with maxCurvature = 1 / minTurningRadius (hybrid_a_star.cpp:214). */
typedef struct pp_smoother_params { /* algo/smoother.h:28-60 */
	float step_tolerance;
	int32_t max_iterations;
	float learning_rate, path_weight, smooth_weight, voronoi_weight, collision_weight, curvature_weight, collision_ratio, max_curvature;
} pp_smoother_params;
typedef struct pp_post_result {
	int32_t n_points;         /* poses of the sampled path (0: the search failed) */
	int32_t smoothing_status; /* Smoother::Status: 0 MaxIteration, 1 StepTolerance, 2 PathSize, -1 Failure; -4: more than max_points samples;
	                           * -2: a smoothed sample fails the vehicle footprint; GetPath() is the sampled path (pp_pipeline_postprocess only) */
	int32_t iterations;
	int32_t reserved;
	double length;            /* length of the composite path */
} pp_post_result;
int pp_planner_postprocess(pp_planner* planner, int32_t n_queries, float path_interpolation, const pp_smoother_params* smoother, int32_t max_points,
	pp_post_result* results_host);
/* sampled path (3 doubles per pose), cusp flags, smoothed path of query q; any pointer may be NULL.  HybridAStar::GetPath() is the
 * smoothed path when smoothing_status >= 0, else the sampled one (hybrid_a_star.cpp:293-303). */
int pp_planner_get_processed_path(pp_planner* planner, int32_t q, double* sampled_host, uint8_t* cusp_host, double* smoothed_host);
/* (row, col) per cell, row-major, (-1, -1) = none: the two label grids of the reference's GVD for maps whose fields were built elsewhere */
int pp_map_upload_nearest_cells(pp_map* map, const int32_t* nearest_obstacle_host, const int32_t* nearest_edge_host);

/* The guard band of the lattice as a contract (pp_query_result::n_lattice_boundary_hits > 0 marks the queries it concerns: some child's
 * DiscretizePose quotient lay within 1e-9 cells of a lattice line, where a last-bit difference between this libm and glibc could
 * choose the other cell).  The host recomputes every created constant-steer node and every LOGGED lattice-line child of query q with
 * glibc along its ancestors (ConstantSteer, models/kinematic_bicycle_model.cpp:5-32) and discretises it (DiscretizePose,
 * algo/hybrid_a_star.h:104-111).  n_cell_mismatches: cells that differ from the device's; n_unverified: flagged events that cannot
 * be recomputed (a Reeds-Shepp child on a lattice line, log entries beyond 64).  Both 0: the query's discrete outputs are certified
 * against the reference's arithmetic; else hand it to the CPU reference.  One-query-per-wave planners only (max_batch <= 64): they
 * keep the tree and the log; flagged queries of a throughput planner / pipeline are re-planned there first (identical results). */
int pp_planner_certify_lattice(pp_planner* planner, int32_t q, int32_t* n_checked, int32_t* n_cell_mismatches, int32_t* n_unverified, double* max_pose_difference);

/* ---- streaming form of HybridAStar::SearchPath: its search stage (algo/hybrid_a_star.cpp:237-257), and by ticket its post-processing
 * (pp_pipeline_postprocess, hybrid_a_star.cpp:260-304) ------------------------------
 * One pipeline per GPU: `capacity` queries in flight (a field slot each: the obstacle-heuristic field of its goal, start / goal /
 * seed, path and Reeds-Shepp log), ObstaclesHeuristic::Update by the wavefront kernel, which hands every finished field to ONE
 * persistent search grid of `search_rows` rows (0 = 4096) through a device-side queue; a row takes the next ready query as soon as
 * its own ends, slots are recycled as results are polled.  No batch boundary: a query that exhausts the lattice (~1 s) holds one
 * row, not a batch's 17 GB of fields.  Results per query are exactly those of pp_planner_search_batch (same kernels' device code).
 * log_expansions != 0 keeps the expansion log per slot (parity tests; 4 B x max_nodes_per_query per slot).
 * 4 <= capacity < 2^20.  The ORDER in which fields are built is the pipeline's own (never a result): queries with a start or goal pose
 * closer than twice the validator's minimum safe radius to an obstacle or to the edge of the state space -- the ones that tend to
 * exhaust the lattice and end a run -- are built ahead of the submissions queued before them (PP_PIPE_URGENT_CLEARANCE=<m>, 0 = in
 * order of submission).  Results arrive in completion order either way.
 * Not thread-safe per pipeline.  Give the HIP runtime a hardware queue per stream (GPU_MAX_HW_QUEUES) before it starts: the pipeline's long launches run on
 * streams of their own, and two streams that share a hardware queue serialise.  pp_pipeline_create CHECKS this (an oversubscribed
 * probe launch on every long-launch stream, a tiny kernel on every other one) and returns PP_ERR_INVALID with a message that names
 * the variable when a stream had to wait; PP_PIPE_ALLOW_SHARED_QUEUES=1 runs regardless (idle waves then leave after PP_PIPE_IDLE_MS). */
typedef struct pp_pipeline pp_pipeline;
int pp_pipeline_create(pp_map* map, const pp_hybrid_params* params, int32_t capacity, int32_t max_nodes_per_query, int32_t search_rows, int32_t log_expansions,
	pp_pipeline** out);
int pp_pipeline_destroy(pp_pipeline* pipeline);
/* Takes up to n_queries queries (as many as there are free slots: *n_accepted; submit the rest after a poll has released slots).
 * tickets_out (may be NULL): one id per accepted query, in input order.  The input arrays are free when the call returns.
 * The map as the kernels see it (bounds, grid pointers, pp_map_set_validator's tunables) is fixed per launch of the persistent search grid: a
 * submission after it changed is refused (PP_ERR_INVALID) while queries are in flight and accepted once they have been polled (the old grid's
 * waves are waited for).  Changing the CONTENTS of the map's grids with queries in flight is the caller's to avoid. */
int pp_pipeline_submit_dev(pp_pipeline* pipeline, int32_t n_queries, const double* starts_dev, const double* goals_dev, const uint64_t* seeds_dev, uint64_t* tickets_out,
	int32_t* n_accepted);
int pp_pipeline_submit(pp_pipeline* pipeline, int32_t n_queries, const double* starts_host, const double* goals_host, const uint64_t* seeds_host, uint64_t* tickets_out,
	int32_t* n_accepted);
/* Completed queries, at most max_results, in completion order; never blocks.  release != 0: their slots are free again at once;
 * release == 0: a slot stays held (pp_pipeline_slot_of + the pp_planner_get_path / get_expanded accessors of pp_pipeline_planner
 * read its path) until pp_pipeline_release. */
int pp_pipeline_poll(pp_pipeline* pipeline, int32_t max_results, uint64_t* tickets_out, pp_query_result* results_out, int32_t release, int32_t* n_out);
int pp_pipeline_release(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets);
/* The plans themselves: GetGraphSearchPath (hybrid_a_star.h:223, a_star.h:254-288) of n completed, held queries (polled with release == 0), start
 * pose first.  poses_host: [n][max_poses][3] doubles (x, y, theta), n_poses_host[i] = nodes on path i (0: no solution; it may exceed max_poses,
 * then only the first max_poses are written).  The row that finishes a query writes its path's poses (up to PP_PIPE_PATH_POSES = 192 per query)
 * into a ring in pinned host memory together with the completion record, so this call copies host memory: no kernel, no device copy (a longer
 * path's remaining records are fetched from the device).  release != 0: the slots are returned like pp_pipeline_release. */
int pp_pipeline_get_paths(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, int32_t max_poses, double* poses_host, int32_t* n_poses_host, int32_t release);
int pp_pipeline_slot_of(pp_pipeline* pipeline, uint64_t ticket); /* -1 unless completed and held */
/* HybridAStar::SearchPath's post-processing (hybrid_a_star.cpp:260-304) of n completed, HELD queries, in the order of `tickets`: what
 * pp_planner_postprocess does for a batch, one workgroup per ticket (k_postprocess_tickets reads the plan of the ticket's field slot and writes at
 * the ticket's position in the list).  results_host[i] (may be NULL) belongs to tickets[i].
 *  - Legal with queries in flight: a held slot is not written until it is released.  The launch runs on the pipeline's control stream with
 *    a copy of the search arguments and the map view of the last submission; only that stream is synchronised, and nothing the search grid
 *    reads is written.
 *  - Footprint: with one set (pp_pipeline_set_footprint) a path whose point checks passed (smoothing_status >= 0 so far) is checked once more
 *    on the device, every sample as the pose (smoothed x, smoothed y, the sample's heading) against the footprint's state predicate; one that
 *    fails gives smoothing_status -2.  The descent itself is unchanged (it knows the point validator only).
 *  - PP_ERR_INVALID, nothing launched, the pipeline usable as before, the message naming the first offending ticket: n < 0 or n > capacity;
 *    max_points outside 8 .. 2048; path_interpolation <= 0; nearest-cell grids missing on the map; a ticket that is unknown, released or still
 *    in flight; a ticket given twice.  n == 0 is PP_OK.
 *  - The pipeline owns the buffers: 58 bytes per sample (ratio 8, sampled pose 24, smoothed pose 24, cusp flag 1, optimise flag 1) x the
 *    largest n x max_points asked so far -- sized by the calls, not by the capacity.  Freeing device memory waits for the whole device, so
 *    a buffer that has to grow while queries are in flight is kept aside and freed by the first later call that finds none in flight (or with
 *    the pipeline): a caller that wants no growth beside a running search makes its largest call first.
 *  - The results stay readable per ticket (pp_pipeline_get_processed_paths) until the ticket is released, by any route, or the next
 *    pp_pipeline_postprocess call that passes validation (one with n == 0 included).
 * smoother == NULL: the defaults of pp_planner_postprocess. */
int pp_pipeline_postprocess(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, float path_interpolation, const pp_smoother_params* smoother, int32_t max_points,
	pp_post_result* results_host);
/* max_points >= 1 is the stride of the caller's arrays (it need not be the max_points of the post-processing call).
 * sampled / cusp / smoothed: [n][max_points][3] doubles / [n][max_points] bytes / [n][max_points][3] doubles, any may be NULL; n_points_host[i] as
 * pp_post_result::n_points (it may exceed max_points, then only the first max_points are written; rows beyond it are unspecified).  Only tickets of
 * the LAST pp_pipeline_postprocess call that are still held: any other is PP_ERR_INVALID.  HybridAStar::GetPath() is the smoothed path when
 * smoothing_status >= 0, else the sampled one.  release != 0: as pp_pipeline_release. */
int pp_pipeline_get_processed_paths(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, int32_t max_points, double* sampled_host, uint8_t* cusp_host,
	double* smoothed_host, int32_t* n_points_host, int32_t release);
/* ---- re-validation of held plans against a changed map, by ticket ------------------------------------------------------------------
 * Is the plan of a completed, HELD query still collision-free on `target` as that map is NOW?  One wave per ticket (k_revalidate_tickets)
 * reads the plan where the search left it -- the path records and the Reeds-Shepp log of the ticket's field slot -- and marches every
 * edge (a constant-steer arc per node, the Reeds-Shepp path of the analytic expansion at the end) with the predicate the search used
 * on it, against the target map's view at the time of the call; then the plan's last pose gets the state check, because IsPathValid
 * (state_validator_occupancy_map.cpp:28-71) never samples ratio 1 of a path.  results_host[i] (may be NULL) belongs to tickets[i].
 *  - target == NULL: the pipeline's own map as it is now (not the view of the last submission, which pp_pipeline_postprocess uses).
 *    Otherwise any pp_map of the same context with a distance grid, of any geometry: bounds, resolution, origins, the distance grid and
 *    pp_map_set_validator's tunables (min_safe_radius, min_path_interpolation_distance) are all the target's.  So a caller may edit map B
 *    while the grid searches map A.  With the pipeline's own map as the target the rule of pp_pipeline_submit_dev holds: changing the
 *    CONTENTS of a map's grids while queries that read them are in flight is the caller's to avoid.
 *  - Without a footprint (pp_pipeline_set_footprint) an edge is checked as pp_check_arcs / pp_check_rs_paths check it and the last pose
 *    as pp_check_states does.  With the pipeline's current footprint: as pp_check_arcs_footprint (gain (float)(1 + |kappa| * rho)),
 *    pp_check_rs_paths_footprint (gain (float)(1 + rho / min_turning_radius)) and pp_check_states_footprint.  Only the footprint's discs
 *    are used; every distance is read from the target's grid, so the footprint need not belong to the target.
 *  - Legal with queries in flight: a held slot is not written until it is released.  The launch runs on the pipeline's control stream
 *    with a copy of the search arguments; only that stream is synchronised, and nothing the search grid reads is written.
 *  - PP_ERR_INVALID, nothing launched, the pipeline usable as before, the message naming the first offending ticket: n < 0 or
 *    n > capacity; a ticket that is unknown, released or still in flight; a ticket given twice; a target of another context; a target
 *    without a distance grid.  n == 0 is PP_OK.
 *  - The pipeline owns the slot list and the result buffer (4 + 32 bytes per ticket of the largest call so far).  One that has to grow while
 *    queries are in flight is kept aside like the post-processing buffers.  The results of the last pp_pipeline_postprocess call are
 *    not touched: pp_pipeline_get_processed_paths works as before.
 * Lengths: `length` is the sequential root-first sum of the edges' lengths, pp_post_result::length bit for bit. */
typedef struct pp_revalidate_result {
	int32_t status;        /* 0 still valid; 1 an edge is blocked; 2 every edge passes, the goal pose fails the state check;
	                          -1 no plan (the search did not succeed); -4 path longer than the planner's path capacity */
	int32_t n_edges;       /* n_path - 1 */
	int32_t blocked_edge;  /* status 1: first blocked edge, root first, 1..n_edges (edge e joins path poses e-1 and e); else 0 */
	float   blocked_ratio; /* status 1: IsPathValid's `last` of that edge; else 1 */
	double  valid_length;  /* metres drivable from the start: lengths of the edges before blocked_edge
	                          + (double)blocked_ratio * that edge's length; == length for status 0 and 2; 0 for status < 0 */
	double  length;        /* composite length, sequential root-first sum */
} pp_revalidate_result;
int pp_pipeline_revalidate(pp_pipeline* pipeline, pp_map* target /* NULL: the pipeline's map as it is now */, int32_t n, const uint64_t* tickets,
	pp_revalidate_result* results_host);
/* The same kernel over the first n_queries queries of the planner's last batch (identity slots), on the planner's stream, with the planner's
 * footprint if it has one (pp_planner_set_footprint).  target == NULL: the planner's own map.  PP_ERR_INVALID: n_queries < 0 or beyond the
 * last batch; a target of another context or without a distance grid; a planner that is a pipeline's buffer set (pp_pipeline_revalidate
 * knows which of its slots are held). */
int pp_planner_revalidate(pp_planner* planner, pp_map* target /* NULL: own map */, int32_t n_queries, pp_revalidate_result* results_host);
/* ---- stamping held plans into a map, by ticket ------------------------------------------------------------------------------------------
 * A STAMP of a plan is the set of cells of a TARGET map covered by the vehicle's discs at sample poses along the plan.  One wave per plan
 * (k_stamp_tickets) reads the plan where the search left it and writes the target's int32 occupancy grid, so a plan becomes part of a map
 * -- a reservation map for the next vehicle of a prioritised planner -- without leaving the device.
 *  Discs.   With a footprint set (pp_pipeline_set_footprint; pp_planner_set_footprint for the batch form) its discs (ox_i, oy_i, r_i); without one
 *           the single disc (0, 0, min_safe_radius) of the pipeline's (planner's) OWN map: the point validator seen as a footprint.  Only the
 *           discs travel, as in re-validation.  Effective radius R_i = (double)r_i + (double)margin.
 *  Edges.   The plan's own path objects: a constant-steer arc per node, then the Reeds-Shepp path of the analytic expansion, numbered root first
 *           1 .. n_path - 1.  S_e = the sequential root-first sum of the lengths of the edges before e (the sum of pp_revalidate_result::length: the
 *           order is part of the result).
 *  Samples. Edge e of length L has n = L > 0 ? (int)ceil(L / spacing) : 0 steps, in double (n is capped at 2^19).  n == 0: one sample at ratio 0;
 *           otherwise the ratios (double)k / (double)n for k = 0 .. n -- both ends, so a junction pose is sampled twice, which is harmless.  The pose
 *           is the path object's interpolation at that ratio (the function post-processing samples with); the sample's arc length is
 *           s = S_e + ratio * L.  A one-pose plan has one sample: its pose, at s = 0.
 *  Window.  Plan i takes part with the samples from_length[i] <= s <= to_length[i], compared in double (NULL array: -inf / +inf): a vehicle that has
 *           driven 12 m reserves [12, 12 + horizon].  An empty window is legal: status 0, n_samples 0.
 *  Centres. Disc i at a sample pose (x, y, theta): the expression of the footprint state check's step 2 -- cx = (x + ox*c) - oy*s,
 *           cy = (y + ox*s) + oy*c with (s, c) = sincos of the unwrapped theta in double; a disc with ox == 0 && oy == 0 uses (x, y) and no trigonometry.
 *  Cells.   Cell (row, col) of the target spans [gx + row res, gx + (row + 1) res) in x and [gy + col res, gy + (col + 1) res) in y, res = (double) of the
 *           target's float resolution, (gx, gy) its grid origin.  It is covered iff its centre (gx + (row + 0.5) res, gy + (col + 0.5) res) satisfies
 *           dx^2 + dy^2 <= R_i^2 in double for some sample in the window and some disc.  Whatever lies outside the target's grid is clipped silently.
 *           No bounds test and no validity test is applied to the poses: a plan is stamped where it lies.
 *  Write.   occupancy[cell] = max(occupancy[cell], values[i]) for every covered cell, values[i] >= 0 (NULL: 0 for every plan; free cells hold -1), by a
 *           vector atomic max: the grid after the call does not depend on the order of plans, samples or lanes.  A target that has no int32 occupancy
 *           grid yet gets one, all -1, as pp_map_set_cells gives it.
 *  Superset. Between two samples the reference point moves at most `spacing`, a disc centre at most spacing * (1 + kappa_max * rho) (rho = the largest
 *           |(ox_i, oy_i)|, kappa_max = 1 / min_turning_radius).  So margin >= 0.5 * spacing * (1 + kappa_max * rho) + res * sqrt(2) / 2 makes the stamp a
 *           superset of every cell the discs touch while they sweep the plan.  The library does not choose a margin for the caller.
 *  Afterwards. What every occupancy writer does: the target's occupancy views are rebuilt (heuristic-clearance views and the tile form's bit rows of
 *           anyone using the target go stale and rebuild as they do after pp_map_set_cells), and the target's stream is drained before the call returns.
 *           The cells written are unknown to the ordered edit record of PP_GVD_REFERENCE_ORDER: the record is dropped and the next update in that mode
 *           re-seeds from the device grid ("every occupied cell, row-major").  The distance grid, the squared distances and the path cost are NOT touched:
 *           the caller runs pp_map_update_gvd[_ex] on the target when it wants the fields to follow.
 *  - target == NULL: the pipeline's own map.  Otherwise any pp_map of the same context, of any geometry.  Stamping another map than the pipeline's own is
 *    legal beside queries in flight (stamp reservation map B while the grid searches map A): the launch runs on the pipeline's control stream with a
 *    copy of the search arguments, only that stream and the target's are synchronised, and a held slot is not written until it is released.
 *  - PP_ERR_INVALID, nothing launched, nothing written, the pipeline usable as before, the message naming the first offending ticket or argument:
 *    n < 0 or n > capacity; a ticket that is unknown, released, still in flight or given twice; a target of another context; NULL params, a spacing that
 *    is not finite and > 0, a margin that is not finite and >= 0; a negative value; a NaN in a window array; the pipeline's OWN map as the target while
 *    pp_pipeline_in_flight() > 0 (the field launches in flight read the occupancy views this call rewrites; held slots do not count).  n == 0 is PP_OK:
 *    nothing is touched.
 *  - The pipeline owns the slot list, the per-ticket arguments and the result buffer (4 + 24 + 32 bytes per ticket of the largest call so far), kept
 *    aside like the post-processing buffers when they have to grow beside queries in flight. */
typedef struct pp_stamp_params {
	double  spacing;  /* > 0, finite, metres */
	float   margin;   /* >= 0, finite */
	int32_t reserved;
} pp_stamp_params;
typedef struct pp_stamp_result {
	int32_t status;      /* 0 stamped (n_samples may be 0); -1 no plan; -4 path longer than the planner's path capacity */
	int32_t n_samples;   /* samples inside the window */
	int32_t cell_box[4]; /* row_min, row_max, col_min, col_max of the cells this plan COVERS inside the target, whatever they held before;
	                        row_min > row_max: none */
	double  length;      /* pp_revalidate_result::length, bit for bit */
} pp_stamp_result;
int pp_pipeline_stamp(pp_pipeline* pipeline, pp_map* target /* NULL: the pipeline's own map */, int32_t n, const uint64_t* tickets, const int32_t* values,
	const double* from_length, const double* to_length, const pp_stamp_params* params, pp_stamp_result* results_host /* may be NULL */);
/* The same kernel over the first n_queries queries of the planner's last batch (identity slots), on the planner's stream, with the planner's
 * footprint if it has one.  PP_ERR_INVALID as above, and for a planner that is a pipeline's buffer set (pp_pipeline_stamp knows which slots are held). */
int pp_planner_stamp(pp_planner* planner, pp_map* target /* NULL: own map */, int32_t n_queries, const int32_t* values, const double* from_length,
	const double* to_length, const pp_stamp_params* params, pp_stamp_result* results_host);
/* ---- locating vehicles on held plans, by ticket -----------------------------------------------------------------------------------------
 * To LOCATE a vehicle on a plan is to find the point of the plan closest to the vehicle's pose: its arc length (what windows pp_pipeline_stamp and
 * what pp_revalidate_result::valid_length is read against), the edge and ratio, the path pose there, the cross-track and heading errors a controller
 * steers on, and the travel direction.  One wave per plan (k_locate_tickets) reads the plan where the search left it.  It reads no map and writes
 * nothing but its own result records, so the call is legal beside queries in flight without exception.  All arithmetic below is in double, in the
 * order written (the library is built without contraction).
 *  Inputs.  poses_host[n][3]: the vehicle poses (x, y, theta), one per ticket.  from_length / to_length: per-ticket windows of arc length with the
 *           stamp's meaning (NULL array: -inf / +inf).  params: spacing (finite, > 0, metres) and heading_weight w (finite, >= 0, metres per radian).
 *  Samples. The stamp's schedule, exactly: edges 1 .. n_path - 1 root first; S_e the sequential root-first sum, so `length` has
 *           pp_revalidate_result::length's bits; edge e of length L has n = L > 0 ? (int)ceil(L / spacing) : 0 steps (capped at 2^19) and the samples
 *           (double)k / (double)n for k = 0 .. n, at arc length s = S_e + ratio * L; a sample takes part iff from <= s <= to.  A one-pose plan has one
 *           sample: its pose, at s = 0.
 *  Cost.    Of a path pose P = (px, py, ptheta) for the vehicle V = (vx, vy, vtheta): ex = vx - px, ey = vy - py; dtheta = a - TWO_PI * rint(a / TWO_PI)
 *           with a = vtheta - ptheta and TWO_PI = 6.283185307179586; c = (ex ex + ey ey) + (w dtheta)(w dtheta).  Candidates are ordered by (c, s): the
 *           smaller c wins, on equal c the smaller s.  One point of the plan has one name: a junction pose is sampled twice, as the end of edge e
 *           (ratio 1) and as the start of edge e + 1 (ratio 0), at one arc length; the second is the candidate, the first only counts in n_samples
 *           (the two poses are equal up to rounding, which must not choose the edge).  A candidate equal in c and s to the best so far does not
 *           replace it (the stage-1 winner stays against the lattice point under it: the same edge, ratio and pose).  The heading term chooses between
 *           the two branches at a cusp or a self-crossing; the window does the same for a caller that knows roughly where the vehicle was.
 *  Stage 1. The winner among the samples inside the window, at arc length s1.  No sample inside the window: status 1.
 *  Stage 2. (Skipped for a one-pose plan.)  delta = spacing / 32, i0 = (int64) floor(s1 / delta).  For i = i0 - 32 .. i0 + 33: u = (double)i * delta is
 *           a candidate iff 0 <= u <= length and from <= u <= to.  Its edge is the largest e with S_e <= u, its ratio L_e > 0 ? (u - S_e) / L_e : 0,
 *           capped at 1, its pose the edge's interpolation at that ratio, its s is u itself.  The lattice i * delta is global, not centred on s1: two
 *           near-equal stage-1 winners next to each other refine over the same points.
 *  Result.  The minimum over the stage-1 winner and the stage-2 candidates.  The resolution along the plan is spacing / 32 where the cost has one
 *           minimum within `spacing` of the best sample.  The library picks no spacing for the caller.
 *  - PP_ERR_INVALID, nothing launched, the pipeline usable as before, the message naming the first offending ticket or argument: n < 0 or
 *    n > capacity; a ticket that is unknown, released, still in flight or given twice; NULL poses_host or NULL params with n > 0; a spacing that is not
 *    finite and > 0, a heading_weight that is not finite and >= 0; a vehicle pose that is not finite; a NaN in a window array.  n == 0 is PP_OK.
 *  - The pipeline owns the slot list, the per-ticket arguments and the result buffer (4 + 40 + 96 bytes per ticket of the largest call so far), kept
 *    aside like the post-processing buffers when they have to grow beside queries in flight. */
typedef struct pp_locate_params {
	double spacing;        /* > 0, finite, metres: the sample spacing of stage 1; the result's resolution is spacing / 32 */
	double heading_weight; /* >= 0, finite, metres per radian */
} pp_locate_params;
typedef struct pp_locate_result {
	int32_t status;        /* 0 located; 1 no sample in the window; -1 no plan; -4 path longer than the planner's path capacity */
	int32_t edge;          /* 1 .. n_path - 1, root first; 0 for a one-pose plan */
	int32_t direction;     /* +1 forward, -1 reverse: the travel direction of the edge at the ratio */
	int32_t n_samples;     /* stage-1 samples inside the window */
	double  s;             /* arc length of the located point, metres from the start */
	double  ratio;         /* position on the edge, 0 .. 1 */
	double  distance;      /* sqrt(ex ex + ey ey) */
	double  along;         /* cos(ptheta) ex + sin(ptheta) ey */
	double  lateral;       /* cos(ptheta) ey - sin(ptheta) ex: positive, the vehicle is to the left of the path pose */
	double  heading_error; /* dtheta */
	double  length;        /* pp_revalidate_result::length, bit for bit */
	double  pose[3];       /* the path pose, theta as interpolated */
} pp_locate_result;        /* 96 bytes; for status != 0 every field but status, n_samples and length is zero */
int pp_pipeline_locate(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, const double* poses_host, const double* from_length, const double* to_length,
	const pp_locate_params* params, pp_locate_result* results_host /* may be NULL */);
/* The same kernel over the first n_queries queries of the planner's last batch (identity slots), on the planner's stream.  PP_ERR_INVALID as above,
 * and for a planner that is a pipeline's buffer set (pp_pipeline_locate knows which slots are held). */
int pp_planner_locate(pp_planner* planner, int32_t n_queries, const double* poses_host, const double* from_length, const double* to_length,
	const pp_locate_params* params, pp_locate_result* results_host);
/* ---- speed profiles along held plans, by ticket ----------------------------------------------------------------------------------------------
 * A SPEED PROFILE of a plan is, for every sample of the stamp's schedule inside a window of arc length, the speed v the vehicle may drive there and
 * the time t at which it arrives there: what a controller that has located its vehicle at s tracks, and what turns "the next 5 seconds" into the
 * window [s, s'] of a stamp.  One wave per plan (k_speed_profile_tickets) reads the plan where the search left it.  It writes nothing but its own
 * buffers, so the call is legal beside queries in flight.  All arithmetic below is in double, in the order written (the library is built without
 * contraction), unless a float is named.
 *  Samples. The stamp's schedule, exactly: edges 1 .. n_path - 1 root first; S_e the sequential root-first sum, so `length` has
 *           pp_revalidate_result::length's bits; edge e of length L has n = L > 0 ? (int)ceil(L / spacing) : 0 steps (capped at 2^19) and the samples
 *           (double)k / (double)n for k = 0 .. n, at arc length s = S_e + ratio * L -- both ends of every edge, so a junction is sampled twice at one s.
 *           A one-pose plan has one sample: its pose, at s = 0.  The samples with from <= s <= to, in schedule order, are the SEQUENCE j = 0 .. N - 1
 *           (one run of the schedule: s does not decrease along it).  N == 0: status 1.  N > max_samples: status -5, and nothing is written to the
 *           plan's sample rows.
 *  Per sample. The pose is the path object's interpolation at the ratio.  The direction dir_j is the path object's travel direction at the ratio; a
 *           sample whose path object reports no motion there (a Reeds-Shepp path of length 0) takes the direction of its predecessor in the sequence,
 *           and has none while no sample of the sequence has moved.  kappa_j >= 0 is |curvature| of a constant-steer edge; on the Reeds-Shepp edge
 *           1 / min_turning_radius on a turning motion and 0 on a straight one, the motion being the one the direction is read from.
 *  Cusp.    Sample j > 0 is a CUSP STOP iff dir_j and dir_{j-1} both exist and differ.  At a junction the second of the two samples is the stop.  A
 *           direction change inside the Reeds-Shepp edge stops at the first sample behind it, up to `spacing` late: the library picks no spacing for
 *           the caller.
 *  Cap.     c = dir_j forward ? v_max_forward : v_max_reverse (a sample without a direction: v_max_reverse).  If kappa_j > 0: c = min(c, sqrt(a_lat /
 *           kappa_j)).  If clearance_gain > 0: c = min(c, v_floor + clearance_gain * (double)cl_j), cl_j the float `clearance` of the footprint state
 *           check of the sample pose ("vehicle footprint", step 3) on the TARGET map's distance grid -- with the holder's footprint its discs, without
 *           one the disc (0, 0, the target's min_safe_radius), as re-validation takes the target's tunables; a pose that fails steps 1-2 (which
 *           includes a negative clearance) has cl_j = 0.  w_j = c * c; then w_j = 0 at a cusp stop; then w_0 = min(w_0, v_start^2); then
 *           w_{N-1} = min(w_{N-1}, v_end^2) (for N == 1 in this order).
 *  Envelope. A_i = w_i - (2 a_acc) s_i, F_j = min_{i <= j} A_i, fwd_j = F_j + (2 a_acc) s_j: what accelerating at a_acc from any earlier sample allows.
 *           B_i = w_i + (2 a_dec) s_i, G_j = min_{i >= j} B_i, bwd_j = G_j - (2 a_dec) s_j: what braking at a_dec for any later sample allows.
 *           e_j = max(0, min(w_j, min(fwd_j, bwd_j))), v_j = sqrt(e_j).  min is exact, so the result does not depend on the order of evaluation.
 *  Time.    t_0 = 0, t_{j+1} = t_j + (dt_j + (dwell if j + 1 is a cusp stop)).  With ds = s_{j+1} - s_j: ds == 0 gives dt_j = 0; else v_j + v_{j+1} > 0 gives
 *           dt_j = (2 ds) / (v_j + v_{j+1}); else both ends stand: x = ds * a_dec / (a_acc + a_dec), dt_j = sqrt(2 x / a_acc) + sqrt(2 (ds - x) / a_dec).
 *           t is the sequential sum in sample order, and the device forms it in that order: t never decreases along the sequence (a sum formed in
 *           another order, e.g. a tree-shaped scan, would differ by a few units of 2^-53 times the number of samples and could step down by an ulp).
 *  - samples_host (may be NULL) is [n][max_samples][3] doubles (s, v, t); rows beyond a plan's n_samples, and every row of a plan whose status is
 *    not 0, are left untouched.  results_host (may be NULL) belongs to tickets[i].
 *  - target == NULL: the pipeline's own map as it is now.  Otherwise a pp_map of the same context, of any geometry.  It is read only when
 *    clearance_gain > 0, and only then must it have a distance grid.
 *  - PP_ERR_INVALID, nothing launched, the pipeline usable as before, the message naming the first offending ticket or argument: n < 0 or
 *    n > capacity; a ticket that is unknown, released, still in flight or given twice; NULL params with n > 0; spacing, v_max_forward, v_max_reverse,
 *    a_acc, a_dec or a_lat not finite and > 0; dwell, clearance_gain or v_floor not finite and >= 0; max_samples < 1; a NaN in a window array; a
 *    v_start or v_end that is not finite and >= 0; a target of another context; with clearance_gain > 0 a target without a distance grid.
 *    n == 0 is PP_OK.
 *  - The pipeline owns the slot list, the per-ticket arguments, the result buffer and the sample rows (4 + 32 + 72 bytes per ticket and 24 bytes per
 *    sample of the largest n x max_samples so far), kept aside like the post-processing buffers when they have to grow beside queries in flight. */
typedef struct pp_speed_profile_params {
	double spacing;        /* > 0, finite, metres: the sample spacing (the stamp's and the locate call's meaning) */
	double v_max_forward;  /* > 0, finite, m/s */
	double v_max_reverse;  /* > 0, finite, m/s */
	double a_acc;          /* > 0, finite, m/s^2 */
	double a_dec;          /* > 0, finite, m/s^2 */
	double a_lat;          /* > 0, finite, m/s^2: v^2 kappa <= a_lat */
	double dwell;          /* >= 0, finite, s: standstill added at every cusp stop */
	double clearance_gain; /* >= 0, finite, 1/s; 0: no clearance term, no map is read */
	double v_floor;        /* >= 0, finite, m/s: the clearance term's cap at clearance 0 */
} pp_speed_profile_params;
typedef struct pp_speed_profile_result {
	int32_t status;          /* 0 profiled; 1 no sample in the window; -1 no plan; -4 path longer than the planner's path capacity;
	                            -5 more than max_samples samples in the window (n_samples says how many) */
	int32_t n_samples;       /* N */
	int32_t n_cusps;         /* cusp stops in the sequence */
	int32_t reserved;
	double  length;          /* pp_revalidate_result::length, bit for bit */
	double  s_first, s_last; /* s_0, s_{N-1} */
	double  duration;        /* t_{N-1}, seconds */
	double  v_peak;          /* max_j v_j */
	double  min_clearance;   /* min_j cl_j as double; +inf when clearance_gain == 0 */
	double  s_min_clearance; /* the smallest s at which it is taken; 0 when clearance_gain == 0 */
} pp_speed_profile_result;   /* 72 bytes; for status != 0 every field but status, n_samples and length is zero */
int pp_pipeline_speed_profile(pp_pipeline* pipeline, pp_map* target /* NULL: the pipeline's map as it is now */, int32_t n, const uint64_t* tickets,
	const double* from_length, const double* to_length, const double* v_start /* NULL: 0 */, const double* v_end /* NULL: 0 */,
	const pp_speed_profile_params* params, int32_t max_samples, double* samples_host /* may be NULL */, pp_speed_profile_result* results_host /* may be NULL */);
/* The same kernel over the first n_queries queries of the planner's last batch (identity slots), on the planner's stream, with the planner's
 * footprint if it has one.  PP_ERR_INVALID as above, and for a planner that is a pipeline's buffer set (pp_pipeline_speed_profile knows which slots
 * are held). */
int pp_planner_speed_profile(pp_planner* planner, pp_map* target /* NULL: own map */, int32_t n_queries, const double* from_length, const double* to_length,
	const double* v_start, const double* v_end, const pp_speed_profile_params* params, int32_t max_samples, double* samples_host,
	pp_speed_profile_result* results_host);
/* ---- space-time conflicts between held plans, by ticket -----------------------------------------------------------------------------------------
 * Do vehicle A and vehicle B, each driving its held plan on the timetable of its speed profile, ever come too close AT THE SAME TIME, and where and
 * when first?  (A stamp reserves space for all time: two vehicles that cross one junction a minute apart block each other there.)  The call takes n
 * plans, a start time for each and a list of pairs; it forms every plan's TRAJECTORY -- its pose at every time of a common lattice -- once
 * (k_trajectory_tickets, one wave per plan) and then the disc separation of every pair over the lattice (k_conflict_pairs, one wave per pair).  No
 * plan data leaves the device.  It reads no map and writes nothing but its own buffers, so the call is legal beside queries in flight.  All
 * arithmetic below is in double, in the order written (the library is built without contraction), unless a float is named.
 *  Profile. A holder remembers its most recent speed-profile call that returned PP_OK: per plan of that call the row, the status and n_samples, and
 *           once its max_samples, a_acc and a_dec; the rows stay where the kernel left them.  A pipeline keys this by ticket, a batch planner by query
 *           index.  A later speed-profile call replaces all of it (one with n == 0 leaves nothing), releasing a ticket drops that ticket's entry, a new
 *           batch on a batch planner drops everything.  The rows of plan i are (s_j, v_j, t_j), j = 0 .. N - 1, t_0 = 0.
 *  Lattice. k0 = (int64) ceil(t_from / dt), k1 = (int64) floor(t_to / dt), both clipped to +-2^62 in double before the conversion; T = k1 - k0 + 1;
 *           tau_m = (double)(k0 + m) * dt for m = 0 .. T - 1.  The lattice is global, not anchored at t_from: two calls with overlapping horizons
 *           look at the same times.
 *  Position. u = tau - t_start[i].  u < 0: absent if hold_before == 0, else at s_0.  u > t_{N-1}: absent if hold_after == 0, else at s_{N-1}.
 *           Otherwise j is the largest index with t_j <= u (binary search; behind equal times the last one).  j == N - 1: s = s_j.  Else, with
 *           ds = s_{j+1} - s_j and delta = u - t_j: ds == 0 gives s = s_j (a junction or a dwell is a standstill).  Else let m be the motion time of
 *           the step, the speed profile's dt_j (without the dwell).  delta >= m gives s = s_{j+1}: the vehicle dwells at the cusp stop.  Else, if
 *           v_j + v_{j+1} > 0: a = (v_{j+1} - v_j) / m and s = s_j + (v_j + (0.5 * a) * delta) * delta.  Else the triangle: x = ds * a_dec / (a_acc +
 *           a_dec), ta = sqrt(2 x / a_acc); delta <= ta gives s = s_j + (0.5 * a_acc) * delta * delta; otherwise r = m - delta and
 *           s = s_{j+1} - (0.5 * a_dec) * r * r.  Last, s is clamped into [s_j, s_{j+1}].
 *  Pose.    e is the largest edge with S_e <= s, ratio = L_e > 0 ? (s - S_e) / L_e : 0, capped at 1 (the locate call's lattice mapping), and the
 *           pose is the path object's interpolation at the ratio.  A one-pose plan gives its pose.  S_e is the sequential root-first sum:
 *           pp_revalidate_result::length's bits.
 *  Separation. The discs are the stamp's: the holder's footprint, else the disc (0, 0, min_safe_radius of the holder's OWN map); their centres are
 *           "vehicle footprint"'s expression on the pose.  The separation of a pair at tau is the minimum over disc a of A and disc b of B of
 *           sqrt(dx dx + dy dy) - ((double)r_a + (double)r_b), (dx, dy) the difference of the centres, A's minus B's.  CONFLICT iff separation < margin.
 *           min_separation is the minimum under the order (separation, tau); the first conflict is the smallest tau in conflict.  Only min and integer
 *           counts are formed across lanes, so no result depends on the order of evaluation.
 *  Between lattice times. A reference point moves at most v_peak * dt between two lattice times, and a disc centre at most v_peak * dt * (1 +
 *           kappa_max * rho), rho the footprint's largest centre offset.  A margin of at least the sum of that bound over the pair's two vehicles
 *           therefore makes "no conflict" hold between the lattice times too.  The library picks neither dt nor margin for the caller.
 *  - pairs (may be NULL) is [n_pairs][2] indices into tickets.  NULL: every pair i < j in row-major order, n_pairs == n (n - 1) / 2; the device
 *    derives the pair from its index and no list is uploaded.
 *  - poses_host (may be NULL) is [n][T][3] doubles (x, y, theta), a NaN in all three where the vehicle is absent; it comes down only when asked for.
 *    plans_host (may be NULL) belongs to tickets[i], results_host (may be NULL) to pairs[p].
 *  - PP_ERR_INVALID, nothing launched, the holder usable as before, the message naming the first offending ticket or argument: n < 0 or
 *    n > capacity; a ticket that is unknown, released, still in flight or given twice; a ticket without a remembered profile ("run speed_profile
 *    first"); NULL t_start or params with n > 0; a t_start that is not finite; t_from, t_to not finite or t_from > t_to; dt not finite and > 0;
 *    margin not finite and >= 0; T < 1 or T > 2^20; a hold flag other than 0 / 1; n_pairs < 0; a pair index outside 0 .. n - 1; a pair (i, i);
 *    pairs == NULL with n_pairs != n (n - 1) / 2.  n == 0 is PP_OK.
 *  - The holder owns the slot list, the per-plan arguments and records (4 + 16 + 32 bytes per plan), the trajectory (48 bytes per plan and lattice
 *    time of the largest n x T so far), the pair list and the pair records (8 + 80 bytes per pair), kept aside like the post-processing buffers when
 *    they have to grow beside queries in flight. */
typedef struct pp_conflict_params {
	double  t_from, t_to;  /* finite, t_from <= t_to: the horizon in absolute seconds */
	double  dt;            /* finite, > 0: the time lattice tau_k = (double)k * dt */
	double  margin;        /* finite, >= 0: conflict iff separation < margin */
	int32_t hold_before;   /* 0: a vehicle is absent before its start; 1: it stands at its first sample */
	int32_t hold_after;    /* 0: absent after its last sample's time; 1: it stands at its last sample */
} pp_conflict_params;      /* 40 bytes */
typedef struct pp_trajectory_result {
	int32_t status;        /* 0; 1 never present on the lattice; -1 the ticket's profile has status != 0 */
	int32_t n_present;
	int32_t first, last;   /* indices 0 .. T-1 of the first / last lattice time it is present; -1, -1 if none */
	double  s_enter, s_leave; /* its arc length at those two times */
} pp_trajectory_result;    /* 32 bytes; for status != 0 n_present, s_enter and s_leave are zero */
typedef struct pp_conflict_result {
	int32_t status;        /* 0 no conflict; 1 conflict; 2 never both present; -1 a plan of the pair has status -1 */
	int32_t n_times;       /* lattice times at which both are present */
	int32_t n_conflict;    /* of them, in conflict */
	int32_t reserved;
	double  t_first;       /* the first lattice time in conflict */
	double  s_first[2];    /* arc lengths of the pair's two plans there */
	double  min_separation;/* over the n_times times; +inf when n_times == 0 */
	double  t_min;         /* the smallest lattice time at which it is taken */
	double  s_min[2];
	double  reserved1;     /* zero: the record is 80 bytes */
} pp_conflict_result;      /* 80 bytes; for status 2 and -1 every field but status is zero, except min_separation = +inf for status 2; for status 0
                              t_first and s_first are zero */
int pp_pipeline_conflicts(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, const double* t_start /* [n], finite */, int32_t n_pairs,
	const int32_t* pairs /* may be NULL */, const pp_conflict_params* params, double* poses_host /* may be NULL */,
	pp_trajectory_result* plans_host /* may be NULL */, pp_conflict_result* results_host /* may be NULL */);
/* The same kernels over the first n_queries queries of the planner's last batch (identity slots; the profiles of the planner's last
 * pp_planner_speed_profile call), on the planner's stream, with the planner's footprint if it has one.  PP_ERR_INVALID as above, and for a planner that
 * is a pipeline's buffer set (pp_pipeline_conflicts knows which slots are held). */
int pp_planner_conflicts(pp_planner* planner, int32_t n_queries, const double* t_start, int32_t n_pairs, const int32_t* pairs,
	const pp_conflict_params* params, double* poses_host, pp_trajectory_result* plans_host, pp_conflict_result* results_host);
/* ---- start delays that clear conflicts, by priority and ticket ------------------------------------------------------------------------------------
 * How long must a lower-priority vehicle wait at its start so that it stays clear of the vehicles above it?  The call takes what a conflict call
 * takes -- n plans, a start time for each, a list of pairs, the lattice -- and a largest delay, and gives every vehicle the smallest whole number
 * of lattice steps to wait so that, on the lattice, it is never closer than the margin to a pair partner of higher priority.  No plan data leaves
 * the device.  It reads no map and writes nothing but its own buffers, so the call is legal beside queries in flight.
 *  Priority. The position in `tickets`: index 0 never yields, and of a pair (a, b) the larger index yields.  The caller sorts: vehicles already
 *           under way go first, with no pairs among themselves.
 *  Lattice. k0, k1, T, tau_m, the profiles, position, pose, discs and separation are exactly "space-time conflicts between held plans"' for
 *           params->lattice.  With D = max_delay_steps (0 <= D, T + D <= 2^20) the call forms the EXTENDED trajectory of every plan: its pose at
 *           the lattice indices k0 - D .. k1, T + D columns, with the undelayed t_start[i] (k_trajectory_tickets, unchanged, on that lattice).
 *  Delay.   A delay is a whole number of lattice steps, and delaying by d steps is an index shift: at lattice time tau_m = (k0 + m) * dt, m = 0 ..
 *           T - 1, vehicle i with delay d_i is where its extended trajectory has column m + D - d_i, and absent exactly where that column is (a NaN).
 *           No time is recomputed, so the result does not depend on the order of evaluation and is reproducible bit for bit from the trajectory.
 *           The effective start reported is t_start[i] + (double)d_i * dt.  A later conflict call with that start forms u = tau - t_start' afresh,
 *           so it agrees with what was decided here to rounding, not bit for bit.
 *  Rule.    Vehicles are decided in index order.  Vehicle i takes the smallest d in 0 .. D such that at every m in 0 .. T - 1 and against every
 *           pair partner j < i that is scheduled (status 0, delay d_j) the two are not both present with separation < margin.  If no d <= D is
 *           clear, its status is 1 and delay_steps = -1, and the vehicles below it are scheduled AS IF IT WERE ABSENT: the caller replans it or calls
 *           again with a larger D.  A plan whose profile or status is bad (pp_trajectory_result::status -1) gets status -1 and is ignored likewise.
 *  Blocker. blocker, t_block and s_block describe the LAST REJECTED candidate: d - 1 for a vehicle that waited d steps, D for status 1.  Of that
 *           candidate's conflicts it is the one with the least key (m, j), compared as integers (m * n + j): blocker = j, an index into tickets,
 *           t_block = tau_m, s_block the arc lengths of i and of j there.  With no rejected candidate blocker is -1 and t_block, s_block are zero.
 *           n_tried is the number of candidates evaluated: delay_steps + 1, or D + 1 for status 1.
 *  Schedule. The order between vehicles is known without device data: level(i) = 0 with no partner j < i, else 1 + max level(j).  The host builds
 *           the levels and each vehicle's list of lower-index partners, and launches k_delay_level once per level, one wave per vehicle of the
 *           level, on the holder's stream; the order of that stream is the only synchronisation.  pairs == NULL lists every pair, so level(i) = i:
 *           n launches of one wave each and n (n - 1) / 2 list entries.  A fleet passes the pairs that can meet.
 *  - PP_ERR_INVALID, nothing launched, the holder usable as before: every refusal of the conflict call (a ticket without a remembered profile: "run
 *    speed_profile first"), and max_delay_steps < 0, T + D > 2^20, reserved != 0.  n == 0 is PP_OK.  results_host may be NULL.
 *  - The holder owns, beside the conflict call's buffers (the trajectory of the largest n x (T + D) so far), 12 + 48 bytes per plan, 4 per listed
 *    pair, kept aside like the post-processing buffers when they have to grow beside queries in flight. */
typedef struct pp_delay_params {
	pp_conflict_params lattice; /* the conflict call's: horizon, dt, margin, hold flags */
	int32_t max_delay_steps;    /* D >= 0, T + D <= 2^20: the delays tried are 0 .. D lattice steps */
	int32_t reserved;           /* zero */
} pp_delay_params;             /* 48 bytes */
typedef struct pp_delay_result {
	int32_t status;        /* 0 scheduled; 1 no delay of 0 .. D steps is clear; -1 the ticket's profile has status != 0 */
	int32_t delay_steps;   /* d; -1 for status 1 and -1 */
	int32_t n_tried;       /* candidates evaluated */
	int32_t blocker;       /* index into tickets of the partner that rejected the last rejected candidate; -1: none was rejected */
	double  t_start;       /* the effective start t_start[i] + (double)d * dt; t_start[i] for status 1; zero for status -1 */
	double  t_block;       /* the lattice time of that candidate's first conflict */
	double  s_block[2];    /* arc lengths of this vehicle and of the blocker there */
} pp_delay_result;        /* 48 bytes; for status -1 every field but status, delay_steps and blocker is zero */
int pp_pipeline_deconflict(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, const double* t_start /* [n], finite */, int32_t n_pairs,
	const int32_t* pairs /* may be NULL */, const pp_delay_params* params, pp_delay_result* results_host /* may be NULL */);
/* The same kernels over the first n_queries queries of the planner's last batch (identity slots; the profiles of the planner's last
 * pp_planner_speed_profile call), on the planner's stream, with the planner's footprint if it has one.  PP_ERR_INVALID as above, and for a planner that
 * is a pipeline's buffer set (pp_pipeline_deconflict knows which slots are held). */
int pp_planner_deconflict(pp_planner* planner, int32_t n_queries, const double* t_start, int32_t n_pairs, const int32_t* pairs,
	const pp_delay_params* params, pp_delay_result* results_host);
/* ---- start delays that clear conflicts and tracked movers, by priority and ticket ----------------------------------------------------------------
 * A person, a manually driven truck, a vehicle held by another pipeline: whatever moves without a plan of this holder is invisible to the delay
 * call above, and a stamp reserves its space for all time.  This call is the delay call with fixed, unprioritised partners added: TRACKS, discs
 * that move along timed waypoints.  Every vehicle gets the smallest start delay at which it is clear of the scheduled vehicles above it AND of
 * every track.  With max_delay_steps == 0 and n_pairs == 0 it is the plain check: does this plan, on its timetable, hit a tracked mover, and when
 * and where first?  With no tracks (tracks == NULL or n_tracks == 0) the delay records are the delay call's, byte for byte.  The definition is
 * that of "start delays that clear conflicts" with the additions below; every expression is in double, in the order written.
 *  Track position. At the lattice time tau = tau_m = (double)(k0 + m) * dt -- the bits the vehicles use -- track k with waypoints (t_j, x_j, y_j),
 *           j = 0 .. W - 1, is absent for tau < t_0 or tau > t_{W-1}; the hold flags are the vehicles' only (a mover that stands is two
 *           waypoints at one place).  Otherwise j is the largest index with t_j <= tau (binary search).  j == W - 1 gives (x_j, y_j).  Else
 *           lam = (tau - t_j) / (t_{j+1} - t_j), x = x_j + lam * (x_{j+1} - x_j), and y likewise.  Tracks are never delayed: they are sampled
 *           on the T columns of k0 .. k1 only (k_track_samples, one wave per track; one array per component, track-major, a NaN where absent).
 *  Separation. Of vehicle i and track k at tau: the minimum over the vehicle's discs a (the conflict call's discs) of sqrt(dx dx + dy dy) -
 *           ((double)r_a + R_k), (dx, dy) the disc's centre minus the track's position, R_k = radii[k].  CONFLICT iff separation < margin.
 *  Rule.    A candidate d of vehicle i is rejected by a scheduled partner j < i as in the delay call, and by track k if at some m the vehicle
 *           (its column m + D - d) and the track are both present in conflict.  In the key order a track is partner n + k: key = m * (n + M) +
 *           partner, so blocker >= n names track blocker - n, and s_block[1] is then 0.0.  With M == 0 this is the delay call's key.  Levels,
 *           n_tried, t_start and the statuses 1 and -1 are unchanged; tracks sit above every vehicle and need no level.  The kernel is
 *           k_delay_level_tracks, launched once per level as k_delay_level is; n_pairs == 0 is one launch.
 *  Records. track_results_host[i * M + k] describes vehicle i against track k at the vehicle's REPORTED candidate: d_i for status 0, D for status
 *           1 (k_track_pairs, one wave per (vehicle, track), launched once behind the last level).  Counts, first conflict and min_separation
 *           are the pair record's, with its two orders; s_first and s_min are the vehicle's arc lengths.  They are computed and copied only when
 *           track_results_host is given and M > 0.
 *  Cost.    O(n (D + 1) T M) separations at worst: every vehicle tries every candidate against every track at every lattice time.  The call has
 *           no list of (vehicle, track) pairs and no broad phase; a caller with many tracks passes the ones that can matter.
 *  - PP_ERR_INVALID, nothing launched, the holder usable as before, the message naming the first offender: everything the delay call refuses;
 *    tracks->reserved != 0; n_tracks < 0 or > 2^16; NULL offsets, waypoints or radii with n_tracks > 0; offsets[0] != 0 or offsets not strictly
 *    increasing; offsets[M] > 2^24; M * T > 2^26; a waypoint value that is not finite; times not strictly increasing within a track; a radius
 *    that is not finite and >= 0.  n == 0 is PP_OK whatever the tracks.
 *  - The holder owns, beside the delay call's buffers, the waypoints, offsets and radii as uploaded (24 bytes per waypoint row, 4 + 8 per
 *    track), 16 bytes per track and lattice time, and 64 bytes per (vehicle, track), kept aside like the others when they have to grow beside
 *    queries in flight. */
typedef struct pp_track_set {
	int32_t n_tracks;          /* M >= 0 */
	int32_t reserved;          /* zero */
	const int32_t* offsets;    /* host, [M + 1]: offsets[0] == 0, strictly increasing; track k owns waypoint rows offsets[k] .. offsets[k+1] - 1 (W_k >= 1) */
	const double*  waypoints;  /* host, [offsets[M]][3]: (t, x, y), all finite, t strictly increasing within a track */
	const double*  radii;      /* host, [M]: finite, >= 0 */
} pp_track_set;              /* 32 bytes */
typedef struct pp_track_result {   /* vehicle i against track k at the vehicle's REPORTED candidate */
	int32_t status;        /* 0 no conflict; 1 conflict; 2 never both present; -1 the vehicle's delay status is -1 */
	int32_t n_times;       /* lattice times at which both are present */
	int32_t n_conflict;    /* of them, in conflict */
	int32_t reserved;
	double  t_first;       /* the first lattice time in conflict */
	double  s_first;       /* the vehicle's arc length there */
	double  min_separation;/* over the n_times times; +inf when n_times == 0 */
	double  t_min;         /* the smallest lattice time at which it is taken */
	double  s_min;         /* the vehicle's arc length there */
	double  reserved1;     /* zero: the record is 64 bytes */
} pp_track_result;        /* 64 bytes; for status 2 and -1 every field but status is zero, except min_separation = +inf for status 2; for status 0
                             t_first and s_first are zero */
int pp_pipeline_deconflict_tracks(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, const double* t_start /* [n], finite */, int32_t n_pairs,
	const int32_t* pairs /* may be NULL */, const pp_delay_params* params, const pp_track_set* tracks /* NULL: M = 0 */,
	pp_delay_result* results_host /* may be NULL */, pp_track_result* track_results_host /* may be NULL; [n][M] */);
/* The same kernels over the first n_queries queries of the planner's last batch, as pp_planner_deconflict is to pp_pipeline_deconflict. */
int pp_planner_deconflict_tracks(pp_planner* planner, int32_t n_queries, const double* t_start, int32_t n_pairs, const int32_t* pairs,
	const pp_delay_params* params, const pp_track_set* tracks, pp_delay_result* results_host, pp_track_result* track_results_host);
/* ---- the pairs that can meet, by a space-time broad phase -----------------------------------------------------------------------------------------
 * The conflict call and the two delay calls take a pair list.  NULL lists every pair -- n (n - 1) / 2 waves for the conflict call, and level(i) = i,
 * n launches one behind the other, for a delay call -- and a list by some heuristic (the nearest by start pose) misses vehicles that start far apart
 * and cross mid-route without anybody saying so.  This call returns a CONSERVATIVE, SORTED, REPRODUCIBLE list from per-plan bounding boxes over blocks
 * of lattice times.  No plan data leaves the device; only the pairs come back.  Every expression is in double, in the order written.
 *  Trajectory. The lattice, profiles, position, pose, hold flags and D = max_delay_steps are those of "start delays that clear conflicts", for
 *           params->delay.  The call forms the extended trajectory exactly as the delay call does: k_trajectory_tickets, unchanged, on k0 - D .. k1,
 *           T + D columns with the undelayed t_start, in the conflict call's buffers.  D = 0 gives a list for pp_*_conflicts.
 *  Boxes.   B = times_per_box, NB = ceil(T / B).  Box b of plan i is the bounding box (xmin, ymin, xmax, ymax) of the reference point (x, y) over the
 *           columns b B .. min(b B + B, T) - 1 + D at which the plan is present (x is not a NaN): the columns a lattice time of block b can read
 *           under any delay 0 .. D (a time m delayed by d reads column m + D - d).  A plan that is present in none of them -- a plan with trajectory
 *           status -1 always -- has a box of four NaNs.  Only min and max are formed, so the boxes do not depend on the order of evaluation.
 *  Reach.   R = max over the holder's discs a (the stamp's: the footprint, or the point validator's one disc) of sqrt(ox_a ox_a + oy_a oy_a) +
 *           (double)r_a, formed on the host; reach = (margin + (R + R)) + 1e-6.  The micrometre covers the rounding of the narrow phase -- disc
 *           centres, differences, the square root, a few ulp of the coordinates -- for coordinates below 10^6 m, where an ulp is about 1e-10 m.
 *  Rule.    Pair (i, j), i < j, is LISTED iff for some b both boxes exist and !(gx > reach) && !(gy > reach), gx = max(xmin_i - xmax_j, xmin_j -
 *           xmax_i) and gy likewise; first_box is the smallest such b.
 *  Guarantee. For any delays d_i, d_j in 0 .. D and any lattice time m: if the discs of i and j are closer than the margin there, (i, j) is listed.
 *           In one line: both columns m + D - d lie in box b = m / B of their plan, two discs closer than the margin have reference points closer
 *           than margin + 2 R, and a box gap on an axis is at most the distance of any two points of the boxes.  Hence pp_*_conflicts (with D = 0),
 *           pp_*_deconflict and pp_*_deconflict_tracks give the same records over the list as over every pair (for the pairs of the list).
 *  Order.   The list is ascending in (i, j), the row-major order of pairs == NULL, and the same bytes on every run: a pair's place is a prefix sum, no
 *           atomic (k_plan_boxes, one wave per plan; k_box_pairs, one wave per row i, once to count and once to fill; k_pair_offsets between them).
 *  - A list longer than max_pairs is PP_OK: the first max_pairs pairs are written, nothing behind them, and the summary says n_found > n_written.
 *  - PP_ERR_INVALID, nothing launched, the holder usable as before: everything the delay call refuses about the tickets, the starts, the lattice and
 *    D (reserved fields included); times_per_box outside 1 .. 2^20; max_pairs < 0; NULL pairs_host with max_pairs > 0; n * NB > 2^26.
 *  - n == 0 and n == 1 are PP_OK with an empty list (n == 0: a summary of zeros, nothing else is looked at but what the delay call refuses).
 *  - Legal beside queries in flight: it writes only its own buffers (32 bytes per plan and box, 8 + 4 + 8 per plan, 12 per pair it writes), kept aside
 *    like the others when they have to grow then.  It synchronises the holder's stream twice: once to learn n_found, once behind the copy. */
typedef struct pp_pair_params {
	pp_delay_params delay;   /* lattice, margin, hold flags, D (0 for a list meant for pp_*_conflicts) */
	int32_t times_per_box;   /* B, 1 .. 2^20 */
	int32_t max_pairs;       /* rows of pairs_host / first_box_host, >= 0 */
} pp_pair_params;            /* 56 bytes */
typedef struct pp_pair_summary {
	int64_t n_found;         /* pairs the rule lists */
	int32_t n_written;       /* min(n_found, max_pairs): the FIRST n_written pairs in order */
	int32_t n_boxes;         /* NB */
	double  reach;
	int32_t n_boxed;         /* plans with at least one box */
	int32_t reserved;        /* zero */
} pp_pair_summary;           /* 32 bytes */
int pp_pipeline_candidate_pairs(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, const double* t_start /* [n], finite */,
	const pp_pair_params* params, int32_t* pairs_host /* [max_pairs][2]; NULL only with max_pairs == 0 */, int32_t* first_box_host /* may be NULL; [max_pairs] */,
	double* boxes_host /* may be NULL; [n][NB][4] */, pp_pair_summary* summary /* may be NULL */);
/* The same kernels over the first n_queries queries of the planner's last batch, as pp_planner_deconflict is to pp_pipeline_deconflict. */
int pp_planner_candidate_pairs(pp_planner* planner, int32_t n_queries, const double* t_start, const pp_pair_params* params, int32_t* pairs_host,
	int32_t* first_box_host, double* boxes_host, pp_pair_summary* summary);
/* ---- timetable look-ups and stops ---------------------------------------------------------------------------------------------------------------
 * The services above read the timetable (s, v, t) a speed-profile call leaves on the device; this call answers questions about it without the rows
 * coming down: where is the vehicle, how fast and on which pose, u seconds after its start; when, on its timetable, is it at arc length s (the s a
 * locate call returned: t_start = now - t re-anchors a vehicle under way for the conflict and delay calls); where does it stand, and for how long.
 * It reads no map and writes only its own buffers.  Every expression is in double, in the order written.
 *  Profile. The holder's most recent speed-profile call, exactly as the conflict call reads it: the rows (s_j, v_j, t_j), j = 0 .. N - 1, a_acc and
 *           a_dec.  A plan whose profile has a status other than 0 gets plan status -1, and every look-up of it status -1.
 *  Stops.   Sample j is a STOP iff v_j == 0.0 -- row 0 and row N - 1 included when they stand.  t_depart = t_j; t_arrive = 0 for j == 0, else
 *           t_{j-1} + step_time(s_j - s_{j-1}, v_{j-1}, v_j) ("speed profiles", Time).  t_j is t_{j-1} + (step_time + dwell), and addition is
 *           monotone, so t_arrive <= t_depart; at a cusp stop they differ by the dwell.  The stops are listed in row order; the FIRST max_stops are
 *           written, nothing behind them, and the list has the same bytes on every run (a stop's place is a count, no atomic).
 *  By time  (by == 1, the value is u).  u < 0: status 1 and the record of u = 0.  u > t_{N-1}: status 2 and the record of u = t_{N-1}.  Otherwise
 *           status 0.  t is the clamped u; j and s are the conflict call's "Position" (the largest j with t_j <= t, the position within the step), so
 *           s has the bits the conflict call's trajectory has for tau - t_start == u.  With delta = t - t_j, ds = s_{j+1} - s_j and m = step_time(ds,
 *           v_j, v_{j+1}), by the first case that applies:
 *             j == N - 1 or ds == 0            v = v_j                      a = 0
 *             delta >= m (the dwell)           v = v_{j+1}                  a = 0
 *             v_j + v_{j+1} > 0 (trapezoid)    a = (v_{j+1} - v_j) / m      v = v_j + a * delta
 *             delta <= ta (triangle)           v = a_acc * delta            a = a_acc           x = ds a_dec / (a_acc + a_dec), ta = sqrt(2 x / a_acc)
 *             otherwise                        v = a_dec * (m - delta)      a = -a_dec
 *  By arc length (by == 0, the value is s).  s < s_0: status 1 and the record of s_0.  s > s_{N-1}: status 2 and the record of s_{N-1}.  Otherwise
 *           status 0.  The reported s is the clamped value.  j is the largest index with s_j <= s -- behind equal arc lengths the LAST row, so a
 *           vehicle found at a cusp stop is on the departure side.  j == N - 1: t = t_j, v = v_j, a = 0.  Otherwise ds = s_{j+1} - s_j > 0,
 *           sigma = s - s_j, m = step_time(ds, v_j, v_{j+1}), and
 *             v_j + v_{j+1} > 0:   a = (v_{j+1} - v_j) / m;  sigma == 0: delta = 0, v = v_j;  else w = v_j v_j + (2 a) sigma (0 if less), v = sqrt(w),
 *                                  delta = (2 sigma) / (v_j + v)
 *             else (triangle)      x = ds a_dec / (a_acc + a_dec);  sigma == 0: delta = 0, v = v_j (= 0), a = a_acc;
 *                                  sigma <= x: delta = sqrt(2 sigma / a_acc), v = a_acc delta, a = a_acc;
 *                                  otherwise r = sqrt(2 (ds - sigma) / a_dec), delta = m - r, v = a_dec r, a = -a_dec
 *           delta is clamped into [0, m] (anything that is not >= 0 is 0), and t = t_j + delta.  t(s) never decreases in s.
 *  Pose.    The conflict call's "Pose" at the reported s: the edge (the largest e with S_e <= s) and the ratio of the locate call's mapping, then the
 *           path object's interpolation.  direction and kappa are the path object's own at that ratio, by the calls the speed profile uses (+1 / -1,
 *           0 where it reports no motion; |curvature|); no direction is carried over from earlier samples.  A one-pose plan gives its pose, edge 0,
 *           ratio 0, direction 0 and kappa 0.
 *  Next stop. next_stop is the index, in the plan's LISTED stops, of the first one with row > j; -1 if none is listed.  When n_stops > max_stops only
 *           the listed ones are searched: a look-up behind the last listed stop says -1 although the plan stops again.  s_to_stop = stop.s - s and
 *           t_to_stop = stop.t_arrive - t; t_remaining = t_{N-1} - t.
 *  - PP_ERR_INVALID, nothing launched, the holder usable as before, the message naming the first offender: everything the conflict call refuses about
 *    n, the tickets and a missing profile ("run speed_profile first"); NULL params, or NULL values_host with n * n_points > 0; by outside {0, 1};
 *    max_stops outside 0 .. 2^16; a reserved field that is not zero; n_points < 0 or n * n_points > 2^26; a value that is not finite.
 *  - Any of the three output pointers may be NULL.  NULL stops_host with max_stops > 0 is allowed: the list is formed (next_stop refers to it) and
 *    counted, not copied.  Rows of stops_host behind a plan's n_listed are left as they are.
 *  - n == 0 is PP_OK.  n_points == 0 gives plans and stops only.
 *  - Legal beside queries in flight: it writes only its own buffers (40 bytes per plan, 32 per plan and listed stop, 8 + 128 per look-up), kept aside
 *    like the others when they have to grow then (k_timetable_tickets, one wave per plan). */
typedef struct pp_timetable_params {
	int32_t by;         /* 0: values are arc lengths s (metres); 1: values are times u since the plan's start (seconds) */
	int32_t max_stops;  /* 0 .. 2^16: rows of stops_host per plan; 0: no stop list */
	int32_t reserved[2];/* zero */
} pp_timetable_params;      /* 16 bytes */
typedef struct pp_timetable_plan {   /* per ticket */
	int32_t status;     /* 0; -1 the ticket's profile has status != 0 */
	int32_t n_samples;  /* N of the profile */
	int32_t n_stops;    /* stops the rule finds */
	int32_t n_listed;   /* min(n_stops, max_stops): the FIRST ones in row order */
	double  s_first, s_last, duration;   /* s_0, s_{N-1}, t_{N-1} */
} pp_timetable_plan;        /* 40 bytes; for status -1 every field but status is zero */
typedef struct pp_timetable_stop {
	int32_t row;        /* j */
	int32_t reserved;
	double  s, t_arrive, t_depart;
} pp_timetable_stop;        /* 32 bytes */
typedef struct pp_timetable_result { /* per look-up */
	int32_t status;     /* 0 inside the profile; 1 before it (the record of its first point); 2 behind it (the record of its last point); -1 plan status -1 */
	int32_t row;        /* j */
	int32_t edge;       /* as pp_locate_result::edge */
	int32_t direction;  /* +1 / -1 / 0: the path object's travel direction at the ratio (0: it reports no motion there) */
	double  s, t, v, a; /* arc length, time since the start, speed, acceleration along the path */
	double  ratio, kappa; /* position on the edge; |curvature| as the speed profile defines kappa_j */
	double  pose[3];
	int32_t next_stop;  /* index into the plan's LISTED stops of the first one with row > j; -1: none listed */
	int32_t reserved;
	double  s_to_stop, t_to_stop; /* stop.s - s, stop.t_arrive - t; zero for next_stop == -1 */
	double  t_remaining;          /* t_{N-1} - t */
	double  reserved1;
} pp_timetable_result;      /* 128 bytes; for status -1 every field but status is zero */
int pp_pipeline_timetable(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, int32_t n_points /* P >= 0 */, const double* values_host /* [n][P], finite */,
	const pp_timetable_params* params, pp_timetable_plan* plans_host /* may be NULL; [n] */, pp_timetable_stop* stops_host /* may be NULL; [n][max_stops] */,
	pp_timetable_result* results_host /* may be NULL; [n][P] */);
/* The same kernel over the first n_queries queries of the planner's last batch, as pp_planner_conflicts is to pp_pipeline_conflicts. */
int pp_planner_timetable(pp_planner* planner, int32_t n_queries, int32_t n_points, const double* values_host, const pp_timetable_params* params,
	pp_timetable_plan* plans_host, pp_timetable_stop* stops_host, pp_timetable_result* results_host);
/* ---- waits at stops that clear conflicts, by priority and ticket ---------------------------------------------------------------------------------
 * A start delay fits a vehicle that has not left; one under way can still wait where its timetable already has it standing: at a cusp stop, a
 * sample with v_j == 0.  This call is the delay call with such waits as further candidates, and with waits already committed as an input, so that
 * it can be called in a loop.  No plan data leaves the device; it reads no map and writes nothing but its own buffers, so the call is legal beside
 * queries in flight.  Every expression is in double, in the order written.
 *  Lattice. Lattice, profiles, position, pose, discs, separation, hold flags, priority, pair list, levels and D = max_delay_steps are exactly those
 *           of "start delays that clear conflicts" for params->delay.  The extended trajectory is k_trajectory_tickets, unchanged, over the lattice
 *           indices k0 - D .. k1: T + D columns, column c with tau_c = (double)(k0 - D + c) * dt and u_c = tau_c - t_start[i].
 *  Stops.   The stops of a plan are the timetable call's: a row j with v_j == 0.0, t_arrive as there.  The ARRIVE COLUMN a of a stop is the smallest
 *           c in 0 .. T + D - 1 with u_c >= t_arrive, or T + D if there is none (u_c never decreases in c: a binary search).  The STANDING POSE of a
 *           stop is the conflict call's "Pose" at s_j; sin and cos of its heading come from the sincos call k_trajectory_tickets makes.  So wherever
 *           a column falls inside the stop's dwell (t_arrive <= u_c <= t_depart) the standing pose equals that column's x, y, theta, s, sin and cos
 *           bit for bit.
 *  Places.  The places of a FREE vehicle are its stops with 0 < row < N - 1 and D <= a < T + D -- stops reached inside the horizon k0 .. k1 -- in row
 *           order, the first max_places of them; a stop reached before k0 or never is skipped and takes no slot of the list.  A free vehicle may
 *           also wait at its START unless no_start_wait[i] != 0: that is place -1, and it is the delay call's delay.
 *  Position under a wait (place, d) at lattice time m, with c = m + D.  No wait, or d == 0: column c.  The start: column c - d.  A stop with arrive
 *           column a: c < a gives column c; a <= c < a + d gives PRESENT, AT THE STANDING POSE, with arc length s_j; otherwise column c - d.  A NaN
 *           column is "absent", as before.  A wait of zero steps is no wait: it is reported as place -2.
 *  Candidates of a free vehicle, in this order: d = 0; then, for d = 1 .. D, the start (if allowed) and then the listed places in ascending order.
 *           The first candidate that is CLEAR is taken: at no m, against no scheduled partner j < i under that partner's own wait, are both present
 *           with separation < margin.  n_tried is the chosen candidate's ordinal plus one, and the number of candidates for status 1.  blocker,
 *           t_block and s_block describe the LAST REJECTED candidate by its least key (m, j), as in the delay call; s_block is read through the
 *           position rule.  (If the d = 0 candidate's least key is at time m0, a candidate (stop q, d) with a_q > m0 + D is where d = 0 was at every
 *           time up to m0, so it is rejected with that same key: the kernel counts and records such a candidate without evaluating it.)
 *  Fixed.   A vehicle with fixed != NULL and fixed[i].row != -2 is not decided: its one candidate is (fixed[i].row, fixed[i].steps).  row == -1 is a
 *           start wait; row >= 0 a wait at that row, which must be a stop (v_row == 0, any row 0 .. N - 1) with a < T + D -- no lower bound on a:
 *           the vehicle may stand there already.  After pp_*_retime ("decided waits written into the timetables") has written a committed wait at a
 *           stop into the rows, that wait needs no fixed entry any more and the vehicle is free again.
 *           A row that does not qualify gives status -2, and the vehicle is ignored like one of status -1.  A
 *           qualifying fixed vehicle is ALWAYS scheduled: status 0 if its candidate is clear, else 2 with the blocker filled in; the vehicles below
 *           see it either way.  Its list of places is its one row (place 0).
 *  Status 1 of a free vehicle: no candidate was clear; the vehicles below it are scheduled as if it were absent, as in the delay call.
 *  Caveat.  A standing pose is not a trajectory column: it lies on the path between columns a - 1 and a.  pp_*_candidate_pairs' guarantee therefore
 *           covers waits only if that call's margin is increased by the longest step, v_peak * dt.  This call does not do that.
 *  - PP_ERR_INVALID, nothing launched, the holder usable as before: every refusal of the delay call; max_places outside 0 .. 2^10; reserved != 0; a
 *    no_start_wait value other than 0 or 1; a fixed row < -2; fixed steps outside 0 .. D.  n == 0 is PP_OK.
 *  - no_start_wait, fixed and each of the three outputs may be NULL.  places_host is [n][max(max_places, 1)]; rows behind a vehicle's n_places are
 *    left as they are.
 *  - The holder owns, beside the delay call's buffers, 8 + 1 + 4 + 16 + 80 bytes per plan and 64 per plan and place, kept aside like the others when
 *    they have to grow beside queries in flight (k_wait_places, one wave per plan; k_wait_level, one wave per vehicle of a level). */
typedef struct pp_wait_params {
	pp_delay_params delay;  /* the delay call's: lattice, margin, hold flags, D */
	int32_t max_places;     /* 0 .. 2^10: stops listed per free vehicle; 0: start waits only */
	int32_t reserved;       /* zero */
} pp_wait_params;           /* 56 bytes */
typedef struct pp_wait_fixed {
	int32_t row;            /* -2 free: the call decides; -1 a wait at the start; >= 0 a wait at that row of the profile */
	int32_t steps;          /* 0 .. D */
} pp_wait_fixed;            /* 8 bytes */
typedef struct pp_wait_result {
	int32_t status;         /* 0 scheduled; 1 no candidate is clear; 2 a fixed wait in conflict (scheduled); -1 the ticket's profile has status != 0;
	                           -2 the fixed row does not qualify */
	int32_t place;          /* -2 no wait; -1 the start; >= 0 the index in the vehicle's listed places */
	int32_t row;            /* the stop's row; else -1 */
	int32_t wait_steps;     /* d; -1 unless scheduled */
	int32_t n_tried;
	int32_t blocker;        /* as pp_delay_result::blocker */
	double  t_start;        /* the effective start t_start[i] + (double)d * dt without a wait (d = 0) and for a start wait, as pp_delay_result::t_start;
	                           t_start[i] itself for a wait at a stop and for status 1 */
	double  t_hold;         /* (double)(k0 - D + a) * dt: the lattice time from which the vehicle stands */
	double  t_resume;       /* (double)(k0 - D + a + d) * dt: the first lattice time it is on its shifted trajectory again */
	double  s_wait;         /* the stop's arc length */
	double  t_block;
	double  s_block[2];
} pp_wait_result;           /* 80 bytes; t_hold, t_resume and s_wait are zero without a wait at a stop; for status -1 and -2 every field but status,
                               place, row, wait_steps and blocker is zero */
typedef struct pp_wait_place {
	int32_t row, column;    /* the stop's row j and its arrive column a */
	double  s, t_arrive;
	double  pose[3];        /* the standing pose */
	double  sin_theta, cos_theta;
} pp_wait_place;            /* 64 bytes */
int pp_pipeline_deconflict_waits(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, const double* t_start /* [n], finite */,
	const uint8_t* no_start_wait /* may be NULL; [n], 0 or 1 */, const pp_wait_fixed* fixed /* may be NULL; [n] */, int32_t n_pairs,
	const int32_t* pairs /* may be NULL */, const pp_wait_params* params, int32_t* n_places_host /* may be NULL; [n] */,
	pp_wait_place* places_host /* may be NULL; [n][max(max_places, 1)] */, pp_wait_result* results_host /* may be NULL; [n] */);
/* The same kernels over the first n_queries queries of the planner's last batch, as pp_planner_deconflict is to pp_pipeline_deconflict. */
int pp_planner_deconflict_waits(pp_planner* planner, int32_t n_queries, const double* t_start, const uint8_t* no_start_wait, const pp_wait_fixed* fixed,
	int32_t n_pairs, const int32_t* pairs, const pp_wait_params* params, int32_t* n_places_host, pp_wait_place* places_host, pp_wait_result* results_host);
/* ---- decided waits written into the timetables, by ticket ----------------------------------------------------------------------------------------
 * pp_*_deconflict_waits tells a vehicle to stand d steps longer at row j of its timetable; the calls above take a start time per plan and nothing
 * else, so none of them learns of it.  This call writes such HOLDS into the (s, v, t) rows themselves: t_j carries the dwell of row j and
 * arrive_time derives the arrival from row j - 1, so standing w seconds longer at row j is t_k += w for every k >= j, and nothing else.  Behind it
 * every service above sees the wait without a changed line: the conflict call verifies a decided schedule, the timetable call reports the true ETA
 * and the longer t_depart, the broad phase boxes the schedule actually driven, and the next pp_*_deconflict_waits round finds the vehicle free, so
 * that it can be given a second wait further on.  Every expression is in double, in the order written.
 *  Profile. The holder's most recent speed-profile call, exactly as the conflict call reads it: the rows (s_j, v_j, t_j), j = 0 .. N - 1, of plan i
 *           where the speed-profile kernel left them, a_acc and a_dec.  The call rewrites their t column IN PLACE and touches nothing else of them.
 *           A plan whose profile has a status other than 0 gets status -1; its holds are skipped, not refused.
 *  Holds.   `holds` is sorted strictly ascending by (plan, row): at most one hold per row.  plan indexes `tickets` (the queries of a batch planner);
 *           row is in 1 .. N - 1 -- row 0 cannot be held, t_0 = 0 is what every reader assumes, and a wait at the start is the caller's t_start, as
 *           before; seconds is finite and may be negative, which shortens a dwell committed earlier.
 *  Validity, on the ORIGINAL rows, per plan, all or nothing.  A hold at row r needs v_r == 0.0 (the timetable call's stop), else the plan gets
 *           status -2; with delta_r = t_r - t_arrive(r) (t_arrive as the timetable call defines it) it needs delta_r + seconds >= 0, else status
 *           -3 (per hold the stop test comes first).  The first offender in list order is reported in bad_hold, and a plan with an offender keeps
 *           every byte of its rows.
 *  Prefix.  P_0 = seconds_0 and P_h = P_{h-1} + seconds_h, summed sequentially in list order over the plan's holds; `held` is the last P.
 *  Rewrite. For row k let h(k) be the last hold of the plan with row <= k.  If there is none the row is untouched; otherwise t'_k = t_k + P_{h(k)}:
 *           one addition per row.  fl(x + P) is monotone in x, so within one hold segment (the rows that share h(k)) the times stay non-decreasing
 *           bit for bit, and in front of the first hold they are untouched.  Across a segment's first row validity bounds the step by rounding only.
 *           A t_arrive recomputed afterwards from row r - 1 may differ from t'_r less the dwell by one ulp, as it already can from the rows as the
 *           speed profile left them (t_j there is t_{j-1} + (step_time + dwell), not t_arrive + dwell).
 *  Accumulation. The call is incremental: a second call adds to what the first left.  Adding -w after +w restores the times to rounding, not bit for
 *           bit.  A new speed-profile call replaces everything.
 *  Consequence. A wait of d steps at the stop of row r decided by pp_*_deconflict_waits on a lattice of step dt is the hold (i, r, (double)d * dt).
 *           A later conflict call forms u = tau - t_start afresh against the retimed rows; it agrees with that call's "Position under a wait" to
 *           rounding, as the delay call's text already says for effective starts.
 *  - PP_ERR_INVALID, nothing launched, the holder usable as before, the message naming the first offender: every refusal of the timetable call about
 *    n, the tickets and a missing profile ("run speed_profile first"); n_holds < 0; NULL holds with n_holds > 0; a plan outside 0 .. n - 1; a row < 1
 *    (for row 0 the message says to shift t_start instead) or, for a plan with a profile, > N - 1; seconds that is not finite; a list that is not
 *    strictly ascending in (plan, row); more than 2^10 holds for one plan.
 *  - n == 0 is PP_OK, whatever the holds.  rows_host, if given, receives the rows after the call in the speed-profile call's layout: the first N rows
 *    of every plan with a profile, nothing else written.  n_holds == 0 with rows_host is the way to read the rows as they are.
 *  - Legal beside queries in flight: it writes only the speed-profile group's own rows and its own buffers (16 + 4 + 40 bytes per plan, 16 per hold),
 *    kept aside like the others when they have to grow then, on the holder's stream, which it alone synchronises (k_retime_tickets, one wave per
 *    plan). */
typedef struct pp_hold {
	int32_t plan;       /* index into the call's tickets (queries) */
	int32_t row;        /* 1 .. N - 1: a stop of that plan's profile */
	double  seconds;    /* finite; added to the dwell of the row */
} pp_hold;                  /* 16 bytes */
typedef struct pp_retime_result {
	int32_t status;     /* 0 applied (also a plan with no hold); -1 the ticket's profile has status != 0; -2 a hold's row is not a stop;
	                       -3 a hold would make a dwell negative */
	int32_t n_holds;    /* holds listed for this plan */
	int32_t first_row;  /* the smallest row whose time changed; -1: none */
	int32_t bad_hold;   /* index into the call's `holds` of the first offending hold (status -2, -3); else -1 */
	double  held;       /* P of the plan's last hold; 0 without one, and for status -2 and -3 */
	double  duration_before, duration;   /* t_{N-1} before and after */
} pp_retime_result;         /* 40 bytes; for status -1 every field but status and bad_hold (-1) is zero */
int pp_pipeline_retime(pp_pipeline* pipeline, int32_t n, const uint64_t* tickets, int32_t n_holds, const pp_hold* holds /* may be NULL iff n_holds == 0 */,
	double* rows_host /* may be NULL; [n][max_samples][3] of the remembered profile call */, pp_retime_result* results_host /* may be NULL; [n] */);
/* The same kernel over the first n_queries queries of the planner's last batch, as pp_planner_timetable is to pp_pipeline_timetable. */
int pp_planner_retime(pp_planner* planner, int32_t n_queries, int32_t n_holds, const pp_hold* holds, double* rows_host, pp_retime_result* results_host);
/* Diagnostics: waves of the search grid that are alive right now (a blocking device-to-host copy; -1 on error). */
int pp_pipeline_alive_waves(pp_pipeline* pipeline);
pp_planner* pp_pipeline_planner(pp_pipeline* pipeline);           /* the buffer set: set_nonholo_table, set_primitives, get_path(slot), ... */
int pp_pipeline_capacity(pp_pipeline* pipeline);
int pp_pipeline_search_rows(pp_pipeline* pipeline);
int pp_pipeline_in_flight(pp_pipeline* pipeline);  /* submitted and not yet polled */
int pp_pipeline_free_slots(pp_pipeline* pipeline);
/* Vehicle footprint for the pipeline's search grid (see "vehicle footprint" above and pp_planner_set_footprint: the same sites ask the
 * footprint, everything else is untouched).  With a footprint the grid is launched as k_hybrid_search_rows_footprint<true>, without one as
 * k_hybrid_search_rows<true>, exactly as before this entry existed.  fp == NULL clears it.  The pipeline holds a reference: the caller
 * may destroy its handle while the footprint is set.
 *  - The waves of the persistent grid keep the kernel and footprint they were launched with, so the call is refused (PP_ERR_INVALID,
 *    "in flight") while pp_pipeline_in_flight() > 0: poll everything first.  Held slots do not count.  An accepted call waits for the old
 *    grid's waves on the pipeline's own streams, then makes one empty dispatch of the new kernel so that a scratch-allocation failure
 *    is an error code.
 *  - A footprint of another map is PP_ERR_INVALID ("another map").
 *  - pp_planner_set_footprint on pp_pipeline_planner() stays refused; the batch planner of the rows kernel takes no footprint either.
 * The search reads the map's float distance grid through the map view, not the footprint's validity bitmaps: a rebuilt distance grid is
 * caught by the view guard of pp_pipeline_submit_dev.  pp_planner_postprocess on a held slot still smooths against the point validator;
 * pp_pipeline_postprocess checks the smoothed samples against the footprint set here (which may be changed while slots are merely held). */
int pp_pipeline_set_footprint(pp_pipeline* pipeline, pp_footprint* fp);
/* Heuristic clearance of the pipeline's field launches (see "heuristic clearance" above): for every goal submitted afterwards a cell is
 * blocked iff occupied[cell] || !(dist[cell] >= radius); the search grid is untouched.  radius == 0 (the default) is the reference's rule.
 *  - Fields already built belong to the old rule, so the call is refused (PP_ERR_INVALID, "in flight") while pp_pipeline_in_flight() > 0:
 *    poll everything first.  Held slots do not count.
 *  - Negative or non-finite radius: PP_ERR_INVALID.
 *  - The map-view guard of pp_pipeline_submit_dev covers the clearance's occupancy views: when the map's distance or occupancy grid has been
 *    written since they were built, they are rebuilt and the wavefront streams are ordered behind the rebuild before the next field launch --
 *    or, with queries in flight, the submission is refused as it is for the map's own view. */
int pp_pipeline_set_heuristic_clearance(pp_pipeline* pipeline, float radius);
int pp_pipeline_heuristic_clearance(pp_pipeline* pipeline, float* radius);
/* Where the queries in flight are, as the row that announced the latest polled result saw the queue's counters (they ride in every
 * completion record): ready = fields built, waiting for a search row; searching = claimed by a row, not yet polled.  A ready queue near 0 = the wavefront stage is the bottleneck, a long one = the search grid is. */
int pp_pipeline_backlog(pp_pipeline* pipeline, int64_t* ready, int64_t* searching);
/* Kernel launch durations since the last call (HIP events on the launching streams), then reset: total milliseconds / launches / goals of
 * the wavefront kernel; total milliseconds / launches of the search grid and its longest launch (a launch that tops up a full grid lasts
 * microseconds, the one that starts it lasts as long as there is work). */
int pp_pipeline_timings(pp_pipeline* pipeline, double* wavefront_ms_total, int64_t* wavefront_launches, int64_t* wavefront_goals, double* search_ms_total,
	int64_t* search_launches, double* search_max_ms);

/* last batch: milliseconds spent in the wavefront kernel and in the search kernel (HIP events) */
int pp_planner_last_timings(pp_planner* planner, float* wavefront_ms, float* search_ms);
/* Diagnostics (never on by default): launch the stamped build of the search kernel and read, per query,
 * 8 shader-clock sums {pop, node load, parent heuristic, children, duplicate scan, insertion, node write, RS}. */
int pp_planner_set_profiling(pp_planner* planner, int32_t enable);
int pp_planner_phase_cycles(pp_planner* planner, int32_t n_queries, uint64_t* cycles_host);

/* ---- a14: Tree::GetNearestNodes (utils/tree.h:73-116; flann exact kNN) ------
 * points/queries: {x, y} doubles; idx/d2: [n_queries][k], ascending squared L2,
 * ties -> lower point index; slots beyond n_points hold -1 / +inf. */
int pp_knn_dev(pp_ctx* ctx, int64_t n_points, const double* points_dev, int64_t n_queries, const double* queries_dev, int32_t k,
	int32_t* idx_dev, double* d2_dev);
int pp_knn(pp_ctx* ctx, int64_t n_points, const double* points_host, int64_t n_queries, const double* queries_host, int32_t k,
	int32_t* idx_host, double* d2_host);

/* ---- a13: RRT / RRT* (algo/rrt.h:55-95, algo/rrt_star.h:53-112) ------------
 * The whole loop runs on the device, one workgroup per tree.  map == NULL: free space
 * (StateValidatorFree).  params = {maxIteration, maxNumberTreeNode, maxConnectionDistance, goalBias[, gamma]}.
 * star: 0 = RRT, 1 = RRT* exactly as the reference (choose-parent among the k = ln N nearest, NO rewire: rrt_star.h:83-97);
 * beyond the reference: 2 = + rewire of the near nodes through the new node with the saving carried down
 * their subtrees (what utils/node.h:203-225 Reparent is for), 3 = the same with a radius near-set, the <= 16 nearest nodes
 * within params[4] * sqrt(ln(n + 1) / (n + 1)). */
typedef struct pp_rrt_result {
	int32_t status;
	int32_t n_nodes;
	int32_t n_path;
	int64_t iterations, n_knn_queries, n_edge_checks;
} pp_rrt_result;
typedef struct pp_rrt pp_rrt;
int pp_rrt_run(pp_ctx* ctx, pp_map* map, const double lower[2], const double upper[2], const double params[4], const double init[2],
	const double goal[2], uint64_t seed, int32_t star, pp_rrt** out, pp_rrt_result* result);
/* n independent problems (own start, goal, seed) on the same map and parameters, one workgroup each, run together. */
int pp_rrt_run_batch(pp_ctx* ctx, pp_map* map, const double lower[2], const double upper[2], const double params[4], int32_t n_problems,
	const double* inits_xy, const double* goals_xy, const uint64_t* seeds, int32_t star, pp_rrt** outs, pp_rrt_result* results);
int pp_rrt_get(pp_rrt* r, double* nodes_xy, int32_t* parents, double* costs, double* path_xy);
int pp_rrt_destroy(pp_rrt* r);

/* ---- a12 / f4: AStarN2 and BidirectionalAStarN2 as a batch on the device ------
 * Engine: algo/a_star.h:326-427 (SearchPath, Expand, ProcessPossibleShortcut; open list order utils/frontier.h:39-48,83-91);
 * propagator: AStarStatePropagatorFcnN2::GetNeighborStates (algo/a_star_n2.cpp:12-28) over the map's occupancy grid; the user
 * functions the reference takes (transition cost, heuristic) are fixed to the ones of its own script
 * (interfaces/python/scripts/example_a_star_grid.py:46-52): Euclidean distance between the two cells, in double.  Other
 * functions stay on the host engine (pathplanning_amd/host/a_star.hpp), which calls back into the caller per edge as the
 * reference does.  bidirectional != 0: BidirectionalAStar::SearchPath (algo/bidirectional_a_star.h:130-196) with the
 * AverageHeuristic pair (:10-39,58-63); inner_goals[q] = {forward heuristic's goal (row, col), reverse heuristic's goal} are the
 * goals held by the two wrapped heuristic objects, which AverageHeuristic never updates (NULL: forward -> goal, reverse -> init).
 * cells are (row, col) pairs.  results[q].status: 0 success, -1 failure (open list empty), -2 open list beyond its workspace
 * (the call then returns PP_ERR_CAPACITY).  paths: [n][max_path][2], root .. goal; in bidirectional mode the meeting cell
 * appears twice as in the reference (GetPath, :66-72); n_path may exceed max_path (then only the first max_path cells are stored).
 * expanded / expanded_reverse (optional): [n][max_expanded][2], states in expansion order = GetExploredStates as a sequence
 * (the root is expanded first; counts may exceed max_expanded likewise). */
typedef struct pp_grid_result {
	int32_t status;
	int32_t n_path;
	int32_t n_expanded;
	int32_t n_expanded_reverse;
	double cost; /* GetOptimalCost; +inf without a path */
} pp_grid_result;
int pp_grid_astar_batch(pp_map* map, int32_t n_queries, const int32_t* init_cells, const int32_t* goal_cells, int32_t bidirectional,
	const int32_t* inner_goals, int32_t max_path, int32_t max_expanded, pp_grid_result* results, int32_t* paths, int32_t* expanded,
	int32_t* expanded_reverse);

#ifdef __cplusplus
}
#endif
#endif /* PP_HIP_H */
