"""ctypes binding of the C ABI (include/pp_hip.h).  No CPU fallback: if libpphip.so is
missing or no GPU is visible, calls fail loudly."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# The streaming pipeline (pp_pipeline_*) keeps several kernels running side by side on their own streams; the runtime maps streams onto
# GPU_MAX_HW_QUEUES hardware queues (read when the HIP runtime starts), and two streams that share a queue serialise.  The library leaves
# that variable to the process's environment: pp_pipeline_create checks whether its streams run side by side and says so if they do not.
# PP_HIP_LIB: another build of the same library (tuning experiments: tools/build_variant.py)
LIB_PATH = os.environ.get("PP_HIP_LIB") or os.path.join(HERE, "lib", "libpphip.so")

c_dp = C.POINTER(C.c_double)
c_fp = C.POINTER(C.c_float)
c_ip = C.POINTER(C.c_int32)
c_u8p = C.POINTER(C.c_uint8)
c_u64p = C.POINTER(C.c_uint64)


class PPError(RuntimeError):
    """A libpphip call returned a negative code (include/pp_hip.h: PP_ERR_INVALID -1, PP_ERR_HIP -2, PP_ERR_NO_DEVICE -3,
    PP_ERR_CAPACITY -4); `code` holds it, the text is pp_last_error()."""
    code = 0


class MapDesc(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("resolution", C.c_float), ("grid_origin", C.c_double * 2),
                ("local_origin", C.c_double * 2), ("lower", C.c_double * 3), ("upper", C.c_double * 3)]


class HybridParams(C.Structure):
    _fields_ = [("wheelbase", C.c_double), ("min_turning_radius", C.c_double), ("direction_switching_cost", C.c_double),
                ("reverse_cost_multiplier", C.c_double), ("forward_cost_multiplier", C.c_double), ("voronoi_cost_multiplier", C.c_double),
                ("num_generated_motion", C.c_uint32), ("spatial_resolution", C.c_double), ("angular_resolution", C.c_double),
                ("heading_alias", C.c_int32), ("negative_k_read", C.c_int32)]

    @classmethod
    def default(cls, **kw):
        # HybridAStar::SearchParameters defaults, algo/hybrid_a_star.h:29-38
        d = dict(wheelbase=2.6, min_turning_radius=2.0, direction_switching_cost=0.0, reverse_cost_multiplier=1.0,
                 forward_cost_multiplier=1.0, voronoi_cost_multiplier=1.0, num_generated_motion=5, spatial_resolution=1.0,
                 angular_resolution=0.0872, heading_alias=1, negative_k_read=1)
        d.update(kw)
        return cls(**d)


class QueryResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_expanded", C.c_int32), ("n_nodes", C.c_int32), ("n_path", C.c_int32), ("cost", C.c_double),
                ("n_rng_draws", C.c_int32), ("n_rs_attempts", C.c_int32), ("n_state_checks", C.c_int64), ("n_path_checks", C.c_int64),
                ("n_lattice_boundary_hits", C.c_int32), ("reserved", C.c_int32)]


# the same record as a numpy dtype (arrays of results without a Python loop)
QUERY_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_expanded", "<i4"), ("n_nodes", "<i4"), ("n_path", "<i4"), ("cost", "<f8"), ("n_rng_draws", "<i4"),
                               ("n_rs_attempts", "<i4"), ("n_state_checks", "<i8"), ("n_path_checks", "<i8"), ("n_lattice_boundary_hits", "<i4"), ("reserved", "<i4")])
assert QUERY_RESULT_DTYPE.itemsize == C.sizeof(QueryResult)

# pp_rs_path (include/pp_hip.h): PathReedsShepp as a 128-byte record
RS_PATH_DTYPE = np.dtype([("start", "<f8", 3), ("final_pose", "<f8", 3), ("motion_length", "<f8", 5), ("steer", "i1", 5), ("direction", "i1", 5),
                          ("reserved", "i1", 6), ("min_turning_radius", "<f8"), ("length", "<f8"), ("cost", "<f4"), ("word", "<i4")])
assert RS_PATH_DTYPE.itemsize == 128


class FootprintDisc(C.Structure):
    """pp_footprint_disc: centre in the vehicle frame (x forward, y left; metres) and radius"""
    _fields_ = [("ox", C.c_double), ("oy", C.c_double), ("r", C.c_float), ("pad", C.c_float)]


PP_FOOTPRINT_MAX_DISCS = 8


class SmootherParams(C.Structure):
    """Smoother::Parameters, algo/smoother.h:28-60"""
    _fields_ = [("step_tolerance", C.c_float), ("max_iterations", C.c_int32), ("learning_rate", C.c_float), ("path_weight", C.c_float), ("smooth_weight", C.c_float),
                ("voronoi_weight", C.c_float), ("collision_weight", C.c_float), ("curvature_weight", C.c_float), ("collision_ratio", C.c_float), ("max_curvature", C.c_float)]


class PostResult(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("smoothing_status", C.c_int32), ("iterations", C.c_int32), ("reserved", C.c_int32), ("length", C.c_double)]


class RevalidateResult(C.Structure):
    """pp_revalidate_result: status 0 still valid, 1 an edge is blocked, 2 only the goal pose fails, -1 no plan, -4 path beyond the path capacity"""
    _fields_ = [("status", C.c_int32), ("n_edges", C.c_int32), ("blocked_edge", C.c_int32), ("blocked_ratio", C.c_float), ("valid_length", C.c_double),
                ("length", C.c_double)]


class StampParams(C.Structure):
    """pp_stamp_params: sample spacing along the plan (> 0, metres) and the margin added to every disc radius (>= 0)"""
    _fields_ = [("spacing", C.c_double), ("margin", C.c_float), ("reserved", C.c_int32)]


class StampResult(C.Structure):
    """pp_stamp_result: status 0 stamped, -1 no plan, -4 path beyond the path capacity; cell_box = (row_min, row_max, col_min, col_max) of the
    cells the plan covers inside the target (row_min > row_max: none)"""
    _fields_ = [("status", C.c_int32), ("n_samples", C.c_int32), ("cell_box", C.c_int32 * 4), ("length", C.c_double)]


class LocateParams(C.Structure):
    """pp_locate_params: sample spacing of stage 1 along the plan (> 0, metres; the result's resolution is spacing / 32) and the weight of the
    heading difference in the cost (>= 0, metres per radian)"""
    _fields_ = [("spacing", C.c_double), ("heading_weight", C.c_double)]


class SpeedProfileParams(C.Structure):
    """pp_speed_profile_params: the sample spacing (> 0, metres), the speed limits by direction (> 0, m/s), the longitudinal and lateral acceleration
    limits (> 0, m/s^2), the dwell at a cusp stop (>= 0, s) and the clearance term cap <= v_floor + clearance_gain * clearance (both >= 0; gain 0: none)"""
    _fields_ = [("spacing", C.c_double), ("v_max_forward", C.c_double), ("v_max_reverse", C.c_double), ("a_acc", C.c_double), ("a_dec", C.c_double),
                ("a_lat", C.c_double), ("dwell", C.c_double), ("clearance_gain", C.c_double), ("v_floor", C.c_double)]


class SpeedProfileResult(C.Structure):
    """pp_speed_profile_result: status 0 profiled, 1 no sample in the window, -1 no plan, -4 path beyond the path capacity, -5 more than max_samples
    samples; the number of samples and cusp stops, the plan's length, the first and last arc length, the arrival time at the last sample, the highest
    speed, and the smallest clearance with the arc length where it is taken (+inf and 0 without a clearance term)"""
    _fields_ = [("status", C.c_int32), ("n_samples", C.c_int32), ("n_cusps", C.c_int32), ("reserved", C.c_int32), ("length", C.c_double), ("s_first", C.c_double),
                ("s_last", C.c_double), ("duration", C.c_double), ("v_peak", C.c_double), ("min_clearance", C.c_double), ("s_min_clearance", C.c_double)]


class ConflictParams(C.Structure):
    """pp_conflict_params: the horizon [t_from, t_to] in absolute seconds, the step dt of the global time lattice k * dt (> 0), the margin (>= 0,
    metres: conflict iff separation < margin) and whether a vehicle stands at its first / last sample before its start / behind its end (0 / 1)"""
    _fields_ = [("t_from", C.c_double), ("t_to", C.c_double), ("dt", C.c_double), ("margin", C.c_double), ("hold_before", C.c_int32), ("hold_after", C.c_int32)]


class TrajectoryResult(C.Structure):
    """pp_trajectory_result: status 0, 1 never present on the lattice, -1 the plan's speed profile has a status other than 0; the number of lattice
    times it is present at, the indices of the first and last of them (-1, -1: none) and its arc length at those two"""
    _fields_ = [("status", C.c_int32), ("n_present", C.c_int32), ("first", C.c_int32), ("last", C.c_int32), ("s_enter", C.c_double), ("s_leave", C.c_double)]


class ConflictResult(C.Structure):
    """pp_conflict_result: status 0 no conflict, 1 conflict, 2 never both present, -1 a plan of the pair has status -1; the lattice times both are
    present at and those in conflict; the first time in conflict with the two arc lengths there; the smallest separation (+inf: never both present),
    the smallest time it is taken at and the two arc lengths there"""
    _fields_ = [("status", C.c_int32), ("n_times", C.c_int32), ("n_conflict", C.c_int32), ("reserved", C.c_int32), ("t_first", C.c_double),
                ("s_first", C.c_double * 2), ("min_separation", C.c_double), ("t_min", C.c_double), ("s_min", C.c_double * 2), ("reserved1", C.c_double)]


class DelayParams(C.Structure):
    """pp_delay_params: the conflict call's parameters (horizon, dt, margin, hold flags) and max_delay_steps, the largest delay tried in lattice steps
    (>= 0, T + max_delay_steps <= 2^20); reserved is zero"""
    _fields_ = [("lattice", ConflictParams), ("max_delay_steps", C.c_int32), ("reserved", C.c_int32)]


class DelayResult(C.Structure):
    """pp_delay_result: status 0 scheduled, 1 no delay of 0 .. max_delay_steps is clear, -1 the plan's speed profile has a status other than 0; the
    delay in lattice steps (-1: none), the candidates evaluated, the partner (an index into the call's plans; -1: none) that rejected the last rejected
    candidate, the effective start, and the lattice time and the two arc lengths of that candidate's first conflict"""
    _fields_ = [("status", C.c_int32), ("delay_steps", C.c_int32), ("n_tried", C.c_int32), ("blocker", C.c_int32), ("t_start", C.c_double), ("t_block", C.c_double),
                ("s_block", C.c_double * 2)]


class PairParams(C.Structure):
    """pp_pair_params: the delay call's parameters (max_delay_steps = 0 for a list meant for a conflict call), times_per_box (B, 1 .. 2^20 lattice times
    per bounding box) and max_pairs, the rows of the caller's pair array"""
    _fields_ = [("delay", DelayParams), ("times_per_box", C.c_int32), ("max_pairs", C.c_int32)]


class PairSummary(C.Structure):
    """pp_pair_summary: the pairs the rule lists, how many of them were written (the first ones in order), the boxes per plan, the reach, the plans with
    at least one box; reserved is zero"""
    _fields_ = [("n_found", C.c_int64), ("n_written", C.c_int32), ("n_boxes", C.c_int32), ("reach", C.c_double), ("n_boxed", C.c_int32), ("reserved", C.c_int32)]


class TimetableParams(C.Structure):
    """pp_timetable_params: by (0: the values are arc lengths, 1: times since the plan's start), max_stops (0 .. 2^16 rows of the stop list per plan);
    reserved is zero"""
    _fields_ = [("by", C.c_int32), ("max_stops", C.c_int32), ("reserved", C.c_int32 * 2)]


class TimetablePlan(C.Structure):
    """pp_timetable_plan: status (0; -1: the profile has a status other than 0), the profile's N, the stops the rule finds and how many of them are
    listed (the first ones in row order), s_0, s_{N-1} and t_{N-1}"""
    _fields_ = [("status", C.c_int32), ("n_samples", C.c_int32), ("n_stops", C.c_int32), ("n_listed", C.c_int32), ("s_first", C.c_double), ("s_last", C.c_double),
                ("duration", C.c_double)]


class TimetableStop(C.Structure):
    """pp_timetable_stop: the row of a standing sample, its arc length, when the vehicle arrives there and when it leaves; reserved is zero"""
    _fields_ = [("row", C.c_int32), ("reserved", C.c_int32), ("s", C.c_double), ("t_arrive", C.c_double), ("t_depart", C.c_double)]


class TimetableResult(C.Structure):
    """pp_timetable_result: one look-up -- status (0 inside the profile, 1 before it, 2 behind it, -1 no profile), row, edge, direction, s, t, v, a,
    ratio, kappa, the pose, the index of the next listed stop (-1: none) with the distance and the time to it, the time to the plan's end"""
    _fields_ = [("status", C.c_int32), ("row", C.c_int32), ("edge", C.c_int32), ("direction", C.c_int32), ("s", C.c_double), ("t", C.c_double), ("v", C.c_double),
                ("a", C.c_double), ("ratio", C.c_double), ("kappa", C.c_double), ("pose", C.c_double * 3), ("next_stop", C.c_int32), ("reserved", C.c_int32),
                ("s_to_stop", C.c_double), ("t_to_stop", C.c_double), ("t_remaining", C.c_double), ("reserved1", C.c_double)]


class WaitParams(C.Structure):
    """pp_wait_params: the delay call's parameters and max_places (0 .. 2^10 stops listed per free vehicle; 0: start waits only); reserved is zero"""
    _fields_ = [("delay", DelayParams), ("max_places", C.c_int32), ("reserved", C.c_int32)]


class WaitFixed(C.Structure):
    """pp_wait_fixed: a wait already committed -- row -2 free (the call decides), -1 a wait at the start, >= 0 a wait at that row of the profile; steps
    0 .. max_delay_steps"""
    _fields_ = [("row", C.c_int32), ("steps", C.c_int32)]


class WaitResult(C.Structure):
    """pp_wait_result: status 0 scheduled, 1 no candidate is clear, 2 a fixed wait in conflict (scheduled), -1 no profile, -2 the fixed row does not
    qualify; the place (-2 no wait, -1 the start, >= 0 the index in the vehicle's listed places), the stop's row, the steps waited, the candidates
    tried, the blocker, the effective start, the lattice times from which the vehicle stands and at which it moves again, the stop's arc length, and
    the lattice time and the two arc lengths of the last rejected candidate's first conflict"""
    _fields_ = [("status", C.c_int32), ("place", C.c_int32), ("row", C.c_int32), ("wait_steps", C.c_int32), ("n_tried", C.c_int32), ("blocker", C.c_int32),
                ("t_start", C.c_double), ("t_hold", C.c_double), ("t_resume", C.c_double), ("s_wait", C.c_double), ("t_block", C.c_double), ("s_block", C.c_double * 2)]


class Hold(C.Structure):
    """pp_hold: `seconds` (finite, may be negative) added to the dwell of the stop at `row` (1 .. N - 1) of plan `plan` of a retime call"""
    _fields_ = [("plan", C.c_int32), ("row", C.c_int32), ("seconds", C.c_double)]


class RetimeResult(C.Structure):
    """pp_retime_result: status 0 applied, -1 no profile, -2 a hold's row is not a stop, -3 a hold would make a dwell negative; the holds listed for the
    plan, the smallest row rewritten (-1: none), the index in the call's list of the first offending hold (-1: none), the sum of the plan's holds, and
    t_{N-1} before and after"""
    _fields_ = [("status", C.c_int32), ("n_holds", C.c_int32), ("first_row", C.c_int32), ("bad_hold", C.c_int32), ("held", C.c_double),
                ("duration_before", C.c_double), ("duration", C.c_double)]


class WaitPlace(C.Structure):
    """pp_wait_place: a stop a vehicle may wait at -- its row, its arrive column in the extended trajectory, its arc length and arrival time, the
    standing pose and the sine and cosine of its heading"""
    _fields_ = [("row", C.c_int32), ("column", C.c_int32), ("s", C.c_double), ("t_arrive", C.c_double), ("pose", C.c_double * 3), ("sin_theta", C.c_double),
                ("cos_theta", C.c_double)]


class TrackSet(C.Structure):
    """pp_track_set: M tracked movers for a deconflict_tracks call -- host pointers to offsets [M + 1] (int32, offsets[0] == 0, strictly increasing),
    waypoints [offsets[M]][3] (t, x, y; t strictly increasing within a track) and radii [M] (>= 0); reserved is zero"""
    _fields_ = [("n_tracks", C.c_int32), ("reserved", C.c_int32), ("offsets", C.c_void_p), ("waypoints", C.c_void_p), ("radii", C.c_void_p)]


class TrackResult(C.Structure):
    """pp_track_result: a vehicle against a track at the vehicle's reported candidate -- status 0 no conflict, 1 conflict, 2 never both present, -1 the
    vehicle's delay status is -1; the lattice times both are present at and those in conflict; the first time in conflict with the vehicle's arc
    length there; the smallest separation (+inf: never both present), the smallest time it is taken at and the vehicle's arc length there"""
    _fields_ = [("status", C.c_int32), ("n_times", C.c_int32), ("n_conflict", C.c_int32), ("reserved", C.c_int32), ("t_first", C.c_double), ("s_first", C.c_double),
                ("min_separation", C.c_double), ("t_min", C.c_double), ("s_min", C.c_double), ("reserved1", C.c_double)]


class LocateResult(C.Structure):
    """pp_locate_result: status 0 located, 1 no sample in the window, -1 no plan, -4 path beyond the path capacity; the located point's edge
    (1 .. n_path - 1; 0 for a one-pose plan), travel direction (+1 / -1), arc length s, ratio on the edge and path pose; the vehicle's distance,
    along / lateral offsets in the path pose's frame (lateral > 0: left of it) and heading error; for status != 0 all of these are zero"""
    _fields_ = [("status", C.c_int32), ("edge", C.c_int32), ("direction", C.c_int32), ("n_samples", C.c_int32), ("s", C.c_double), ("ratio", C.c_double),
                ("distance", C.c_double), ("along", C.c_double), ("lateral", C.c_double), ("heading_error", C.c_double), ("length", C.c_double), ("pose", C.c_double * 3)]


class GridResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_path", C.c_int32), ("n_expanded", C.c_int32), ("n_expanded_reverse", C.c_int32), ("cost", C.c_double)]


class RrtResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_nodes", C.c_int32), ("n_path", C.c_int32), ("iterations", C.c_int64),
                ("n_knn_queries", C.c_int64), ("n_edge_checks", C.c_int64)]


_lib = None


def load():
    """Loads libpphip.so; raises if it has not been built (run `python -m pathplanning_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PPError("libpphip.so not found at %s -- build it with `python -m pathplanning_amd.build` (hipcc, gfx950). "
                      "There is no CPU fallback." % LIB_PATH)
    try:
        # PyTorch ships its own copy of the HIP / HSA runtime.  Whichever copy initialises second in a process sees no
        # device, so when torch is installed it goes first and libpphip binds to the copy torch loaded.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.pp_last_error.restype = C.c_char_p
    L.pp_obstacle_heuristic_workspace_bytes.restype = C.c_int64
    vp = C.c_void_p
    L.pp_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.pp_ctx_destroy.argtypes = [vp]
    L.pp_ctx_synchronize.argtypes = [vp]
    L.pp_ctx_is_idle.argtypes = [vp, C.POINTER(C.c_int32)]
    L.pp_ctx_timer_start.argtypes = [vp]
    L.pp_ctx_timer_stop.argtypes = [vp, c_fp]
    L.pp_map_create.argtypes = [vp, C.POINTER(MapDesc), C.POINTER(vp)]
    L.pp_map_destroy.argtypes = [vp]
    L.pp_map_upload_dist2.argtypes = [vp, vp]
    L.pp_map_upload_occupancy.argtypes = [vp, vp]
    L.pp_map_upload_path_cost.argtypes = [vp, vp]
    L.pp_map_set_validator.argtypes = [vp, C.c_float, C.c_float]
    L.pp_map_download_distance.argtypes = [vp, vp]
    L.pp_check_states.argtypes = [vp, C.c_int64, vp, vp]
    L.pp_check_states_dev.argtypes = [vp, C.c_int64, vp, vp]
    L.pp_check_states_fused_dev.argtypes = [vp, C.c_int64, C.c_uint64, vp]
    L.pp_check_arcs.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.pp_check_arcs_dev.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.pp_check_segments.argtypes = [vp, C.c_int64, vp, vp, vp]
    L.pp_check_segments_dev.argtypes = [vp, C.c_int64, vp, vp, vp]
    L.pp_rollout_children.argtypes = [vp, C.POINTER(HybridParams), C.c_int32, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.pp_rollout_children_dev.argtypes = [vp, C.POINTER(HybridParams), C.c_int32, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.pp_map_upload_distance.argtypes = [vp, vp]
    L.pp_map_rasterize_segments.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp]
    L.pp_map_download_occupancy.argtypes = [vp, vp]
    L.pp_map_update_gvd.argtypes = [vp, C.c_float, C.c_float, vp]
    L.pp_map_update_gvd_ex.argtypes = [vp, C.c_float, C.c_float, C.c_int32, vp]
    L.pp_map_download_gvd.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.pp_path_cost_update.argtypes = [vp, vp, vp, C.c_float, C.c_float, vp]
    L.pp_rs_connect.argtypes = [vp, C.c_int64, vp, vp, C.c_double, C.c_float, C.c_float, C.c_float, vp]
    L.pp_rs_path_interpolate.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    L.pp_rs_path_truncate.argtypes = [vp, C.c_int64, vp, vp, C.c_int32]
    L.pp_rs_path_cusps.argtypes = [vp, C.c_int64, vp, vp, vp]
    L.pp_check_rs_paths.argtypes = [vp, C.c_int64, vp, vp, vp]
    L.pp_check_rs_paths_dev.argtypes = [vp, C.c_int64, vp, vp, vp]
    L.pp_check_se2_paths.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    L.pp_footprint_create.argtypes = [vp, C.c_int32, vp, C.POINTER(vp)]
    L.pp_footprint_destroy.argtypes = [vp]
    L.pp_footprint_cover_rectangle.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int32, vp]
    L.pp_check_states_footprint.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
    L.pp_check_states_footprint_dev.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.pp_check_arcs_footprint.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.pp_check_arcs_footprint_dev.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.pp_check_rs_paths_footprint.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
    L.pp_check_rs_paths_footprint_dev.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
    L.pp_check_se2_paths_footprint.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp]
    L.pp_planner_set_footprint.argtypes = [vp, vp]
    L.pp_pipeline_set_footprint.argtypes = [vp, vp]
    L.pp_rs_solve.argtypes = [vp, C.c_int64, vp, vp, C.c_double, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp]
    L.pp_rs_solve_dev.argtypes = [vp, C.c_int64, vp, vp, C.c_double, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp]
    L.pp_nonholo_dims.argtypes = [vp, vp, C.POINTER(HybridParams), vp, vp]
    L.pp_nonholo_build.argtypes = [vp, vp, vp, C.POINTER(HybridParams), vp]
    L.pp_nonholo_build_dev.argtypes = [vp, vp, vp, C.POINTER(HybridParams), vp]
    L.pp_obstacle_heuristic.argtypes = [vp, C.c_int32, vp, vp]
    L.pp_obstacle_heuristic_dev.argtypes = [vp, C.c_int32, vp, vp]
    L.pp_obstacle_heuristic_clearance.argtypes = [vp, C.c_float, C.c_int32, vp, vp]
    L.pp_obstacle_heuristic_clearance_dev.argtypes = [vp, C.c_float, C.c_int32, vp, vp]
    L.pp_heuristic_clearance_build_ms.argtypes = [vp, C.c_float, C.c_int32, c_fp]
    L.pp_planner_set_heuristic_clearance.argtypes = [vp, C.c_float]
    L.pp_planner_heuristic_clearance.argtypes = [vp, c_fp]
    L.pp_pipeline_set_heuristic_clearance.argtypes = [vp, C.c_float]
    L.pp_pipeline_heuristic_clearance.argtypes = [vp, c_fp]
    L.pp_obstacle_heuristic_workspace_bytes.argtypes = [vp]
    L.pp_obstacle_heuristic_profile.argtypes = [vp, C.c_int32, vp, vp]
    L.pp_obstacle_heuristic_tiles_stats.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
    L.pp_planner_create.argtypes = [vp, C.POINTER(HybridParams), C.c_int32, C.c_int32, C.POINTER(vp)]
    L.pp_planner_search_rows.argtypes = [vp]
    L.pp_planner_debug_nodes.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
    L.pp_planner_debug_node_actions.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
    L.pp_planner_certify_lattice.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
    L.pp_planner_create_ex.argtypes = [vp, C.POINTER(HybridParams), C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.pp_planner_destroy.argtypes = [vp]
    L.pp_planner_set_nonholo_table.argtypes = [vp, vp]
    L.pp_planner_get_nonholo_table.argtypes = [vp, vp]
    L.pp_planner_num_primitives.argtypes = [vp]
    L.pp_planner_set_primitives.argtypes = [vp, C.c_int32, vp]
    L.pp_planner_search_batch.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
    L.pp_planner_search_batch_dev.argtypes = [vp, C.c_int32, vp, vp, vp]
    L.pp_planner_fetch_results.argtypes = [vp, C.c_int32, vp]
    L.pp_planner_get_path.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
    L.pp_planner_get_expanded.argtypes = [vp, C.c_int32, vp]
    L.pp_planner_get_obstacle_field.argtypes = [vp, C.c_int32, vp]
    L.pp_pipeline_create.argtypes = [vp, C.POINTER(HybridParams), C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
    L.pp_pipeline_destroy.argtypes = [vp]
    L.pp_pipeline_submit_dev.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
    L.pp_pipeline_submit.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
    L.pp_pipeline_poll.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp]
    L.pp_pipeline_release.argtypes = [vp, C.c_int32, vp]
    L.pp_pipeline_get_paths.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, vp, C.c_int32]
    L.pp_pipeline_slot_of.argtypes = [vp, C.c_uint64]
    L.pp_pipeline_postprocess.argtypes = [vp, C.c_int32, vp, C.c_float, vp, C.c_int32, vp]
    L.pp_pipeline_get_processed_paths.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, C.c_int32]
    L.pp_pipeline_revalidate.argtypes = [vp, vp, C.c_int32, vp, vp]
    L.pp_planner_revalidate.argtypes = [vp, vp, C.c_int32, vp]
    L.pp_pipeline_stamp.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, C.POINTER(StampParams), vp]
    L.pp_planner_stamp.argtypes = [vp, vp, C.c_int32, vp, vp, vp, C.POINTER(StampParams), vp]
    L.pp_pipeline_locate.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.POINTER(LocateParams), vp]
    L.pp_planner_locate.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(LocateParams), vp]
    L.pp_pipeline_speed_profile.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(SpeedProfileParams), C.c_int32, vp, vp]
    L.pp_planner_speed_profile.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, C.POINTER(SpeedProfileParams), C.c_int32, vp, vp]
    L.pp_pipeline_conflicts.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, C.POINTER(ConflictParams), vp, vp, vp]
    L.pp_planner_conflicts.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, C.POINTER(ConflictParams), vp, vp, vp]
    L.pp_pipeline_deconflict.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, C.POINTER(DelayParams), vp]
    L.pp_planner_deconflict.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, C.POINTER(DelayParams), vp]
    L.pp_pipeline_deconflict_tracks.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, C.POINTER(DelayParams), C.POINTER(TrackSet), vp, vp]
    L.pp_planner_deconflict_tracks.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, C.POINTER(DelayParams), C.POINTER(TrackSet), vp, vp]
    L.pp_pipeline_candidate_pairs.argtypes = [vp, C.c_int32, vp, vp, C.POINTER(PairParams), vp, vp, vp, C.POINTER(PairSummary)]
    L.pp_planner_candidate_pairs.argtypes = [vp, C.c_int32, vp, C.POINTER(PairParams), vp, vp, vp, C.POINTER(PairSummary)]
    L.pp_pipeline_timetable.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, C.POINTER(TimetableParams), vp, vp, vp]
    L.pp_planner_timetable.argtypes = [vp, C.c_int32, C.c_int32, vp, C.POINTER(TimetableParams), vp, vp, vp]
    L.pp_pipeline_deconflict_waits.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, C.POINTER(WaitParams), vp, vp, vp]
    L.pp_planner_deconflict_waits.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, C.POINTER(WaitParams), vp, vp, vp]
    L.pp_pipeline_retime.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, vp, vp]
    L.pp_planner_retime.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.pp_pipeline_timings.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.pp_pipeline_backlog.argtypes = [vp, vp, vp]
    L.pp_pipeline_planner.argtypes = [vp]
    L.pp_pipeline_planner.restype = vp
    for f in ("pp_pipeline_capacity", "pp_pipeline_search_rows", "pp_pipeline_in_flight", "pp_pipeline_free_slots", "pp_pipeline_alive_waves"):
        getattr(L, f).argtypes = [vp]
    L.pp_planner_postprocess.argtypes = [vp, C.c_int32, C.c_float, vp, C.c_int32, vp]
    L.pp_planner_get_processed_path.argtypes = [vp, C.c_int32, vp, vp, vp]
    L.pp_map_upload_nearest_cells.argtypes = [vp, vp, vp]
    L.pp_planner_last_timings.argtypes = [vp, c_fp, c_fp]
    L.pp_planner_set_profiling.argtypes = [vp, C.c_int32]
    L.pp_planner_phase_cycles.argtypes = [vp, C.c_int32, vp]
    L.pp_knn.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, C.c_int32, vp, vp]
    L.pp_knn_dev.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, C.c_int32, vp, vp]
    L.pp_rrt_run.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_int32, C.POINTER(vp), C.POINTER(RrtResult)]
    L.pp_rrt_run_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.POINTER(vp), C.POINTER(RrtResult)]
    L.pp_rrt_get.argtypes = [vp, vp, vp, vp, vp]
    L.pp_rrt_destroy.argtypes = [vp]
    L.pp_planner_start_after_fields_of.argtypes = [vp, vp]
    L.pp_grid_astar_batch.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.POINTER(GridResult), vp, vp, vp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        e = PPError("libpphip error %d: %s" % (rc, load().pp_last_error().decode()))
        e.code = rc
        raise e


def ptr(a):
    """Host pointer of a contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)
