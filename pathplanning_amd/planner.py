"""Host-side mirror of the reference's operator interface for the hot path, on top of the C ABI.

Class / method names follow the reference's pybind11 module (interfaces/python/src/pyplanning.cpp)
where a counterpart exists: StateValidatorOccupancyMap.is_state_valid / is_path_valid,
HybridAStar.set_init_state / set_goal_state / search_path / get_path, Status.  Batched entry
points are the MI355X-native addition.  Everything computes on the GPU through libpphip.so;
nothing here falls back to the CPU.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import (RS_PATH_DTYPE, ConflictParams, ConflictResult, DelayParams, DelayResult, FootprintDisc, Hold, HybridParams, LocateParams, LocateResult, MapDesc, PairParams, PairSummary, PostResult, QueryResult, RetimeResult, RevalidateResult,
                   SmootherParams, SpeedProfileParams, SpeedProfileResult, StampParams, StampResult, TimetableParams, TimetablePlan, TimetableResult, TimetableStop, TrackResult, TrackSet, TrajectoryResult, WaitFixed, WaitParams, WaitPlace, WaitResult,
                   check, ptr)


class Status:
    """algo/path_planner.h:9-12"""
    SUCCESS = 0
    FAILURE = -1


def _f64(a, cols):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a.reshape(-1, cols)


def _is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _dev_ptr(t):
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


class Context:
    """One device + one HIP stream.  `stream` may be a raw hipStream_t (int), e.g.
    torch.cuda.current_stream().cuda_stream, so that torch events see the work."""

    def __init__(self, device=0, stream=None):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.pp_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device

    def synchronize(self):
        check(self.lib.pp_ctx_synchronize(self.h))

    def is_idle(self):
        """True when everything enqueued on this context's stream has completed (non-blocking)."""
        idle = C.c_int32(0)
        check(self.lib.pp_ctx_is_idle(self.h, C.byref(idle)))
        return bool(idle.value)

    def timer_start(self):
        check(self.lib.pp_ctx_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        check(self.lib.pp_ctx_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.lib.pp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OccupancyMapSet:
    """Device-resident data of one OccupancyMap + GVD: squared-distance grid, occupancy, Voronoi
    potential, plus the StateSpaceSE2 bounds (state_validator/occupancy_map.h:122-133)."""

    def __init__(self, ctx, lower, upper, resolution, rows, cols, grid_origin, local_origin=(0.0, 0.0)):
        self.ctx = ctx
        self.lib = ctx.lib
        self.lower = np.asarray(lower, dtype=np.float64)
        self.upper = np.asarray(upper, dtype=np.float64)
        self.resolution = np.float32(resolution)
        self.rows, self.cols = int(rows), int(cols)
        self.grid_origin = np.asarray(grid_origin, dtype=np.float64)
        d = MapDesc()
        d.rows, d.cols, d.resolution = self.rows, self.cols, float(self.resolution)
        d.grid_origin[:] = list(self.grid_origin)
        d.local_origin[:] = list(local_origin)
        d.lower[:] = list(self.lower)
        d.upper[:] = list(self.upper)
        self.desc = d
        h = C.c_void_p()
        check(self.lib.pp_map_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h

    @classmethod
    def from_bounds(cls, ctx, lower, upper, resolution):
        """Sizes the grid like StateValidatorOccupancyMap's constructor + OccupancyMap::InitializeSize
        (state_validator_occupancy_map.cpp:6-13, occupancy_map.cpp:6-14): float width/height."""
        lower = np.asarray(lower, dtype=np.float64)
        upper = np.asarray(upper, dtype=np.float64)
        res = np.float32(resolution)
        width = np.float32(upper[0] - lower[0])
        height = np.float32(upper[1] - lower[1])
        origin = (-float(width) / 2.0, -float(height) / 2.0)
        rows = int(math.ceil(float(np.float32(width / res))))
        cols = int(math.ceil(float(np.float32(height / res))))
        return cls(ctx, lower, upper, res, rows, cols, origin)

    def upload_dist2(self, d2):
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        assert d2.shape == (self.rows, self.cols)
        check(self.lib.pp_map_upload_dist2(self.h, ptr(d2)))

    def upload_distance(self, dist):
        """float distance grid in metres, as ObstacleDistanceMap::GetDistanceToNearestObstacle returns it (gvd.h:38)"""
        dist = np.ascontiguousarray(dist, dtype=np.float32)
        assert dist.shape == (self.rows, self.cols)
        check(self.lib.pp_map_upload_distance(self.h, ptr(dist)))

    # ---- map authoring / field construction on the device ----
    def rasterize_segments(self, p0, p1, value):
        """Shape::RasterizeLine for each world segment p0[i] -> p1[i]; writes `value` (obstacle id, or -1 to remove).  Returns cells written."""
        a, b = _f64(p0, 2), _f64(p1, 2)
        n = C.c_int32(0)
        check(self.lib.pp_map_rasterize_segments(self.h, len(a), ptr(a), ptr(b), int(value), C.byref(n)))
        return n.value

    def add_polygon(self, vertices, pose, value):
        """PolygonShape::GetGridCellsPosition (obstacle.cpp:77-93): vertices rotated / translated by `pose` on the host, edges
        rasterised on the device."""
        v = _f64(vertices, 2)
        c, s_ = math.cos(pose[2]), math.sin(pose[2])
        w = np.column_stack([c * v[:, 0] - s_ * v[:, 1] + pose[0], s_ * v[:, 0] + c * v[:, 1] + pose[1]])
        return self.rasterize_segments(w, np.roll(w, -1, axis=0), value)

    def download_occupancy(self):
        occ = np.empty((self.rows, self.cols), dtype=np.int32)
        check(self.lib.pp_map_download_occupancy(self.h, ptr(occ)))
        return occ

    GVD_EXACT_EDT, GVD_REFERENCE_ORDER = 0, 1

    def update_gvd(self, alpha=20.0, d_max=30.0, mode=0):
        """GVD::Update from the device occupancy grid.  mode GVD_REFERENCE_ORDER: the reference's brushfire replayed over the ordered cell
        edits (grids bit-identical to the reference's, incremental after the first call; returns heap pops so far); GVD_EXACT_EDT
        (default): exact Euclidean transform on the device (returns the number of device passes)."""
        it = C.c_int32(0)
        check(self.lib.pp_map_update_gvd_ex(self.h, C.c_float(alpha), C.c_float(d_max), int(mode), C.byref(it)))
        return it.value

    def download_gvd(self):
        shape = (self.rows, self.cols)
        out = dict(d2=np.empty(shape, np.int32), nearest_obstacle=np.empty(shape + (2,), np.int32), voronoi_edge=np.empty(shape, np.uint8),
                   voronoi_d2=np.empty(shape, np.int32), nearest_edge=np.empty(shape + (2,), np.int32), path_cost=np.empty(shape, np.float32))
        check(self.lib.pp_map_download_gvd(self.h, ptr(out["d2"]), ptr(out["nearest_obstacle"]), ptr(out["voronoi_edge"]), ptr(out["voronoi_d2"]),
                                           ptr(out["nearest_edge"]), ptr(out["path_cost"])))
        return out

    def path_cost_update(self, obstacle_d2, voronoi_d2, alpha=20.0, d_max=30.0):
        """PathCostMap::Update (gvd.cpp:266-283) over two squared-distance grids; becomes the map's path cost."""
        a = np.ascontiguousarray(obstacle_d2, dtype=np.int32)
        b = np.ascontiguousarray(voronoi_d2, dtype=np.int32)
        out = np.empty((self.rows, self.cols), dtype=np.float32)
        check(self.lib.pp_path_cost_update(self.h, ptr(a), ptr(b), C.c_float(alpha), C.c_float(d_max), ptr(out)))
        return out

    def upload_nearest_cells(self, nearest_obstacle, nearest_edge):
        """(rows, cols, 2) int grids: GVD::GetNearestObstacleCell / GetNearestVoronoiEdgeCell per cell (the smoother reads them)"""
        a = np.ascontiguousarray(nearest_obstacle, dtype=np.int32)
        b = np.ascontiguousarray(nearest_edge, dtype=np.int32)
        assert a.shape == b.shape == (self.rows, self.cols, 2)
        check(self.lib.pp_map_upload_nearest_cells(self.h, ptr(a), ptr(b)))

    def upload_occupancy(self, occ):
        occ = np.ascontiguousarray(occ, dtype=np.int32)
        assert occ.shape == (self.rows, self.cols)
        check(self.lib.pp_map_upload_occupancy(self.h, ptr(occ)))

    def upload_path_cost(self, cost):
        cost = np.ascontiguousarray(cost, dtype=np.float32)
        assert cost.shape == (self.rows, self.cols)
        check(self.lib.pp_map_upload_path_cost(self.h, ptr(cost)))

    def download_distance(self):
        out = np.empty((self.rows, self.cols), dtype=np.float32)
        check(self.lib.pp_map_download_distance(self.h, ptr(out)))
        return out

    def close(self):
        if self.h:
            self.lib.pp_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Footprint:
    """A vehicle footprint (include/pp_hip.h, "vehicle footprint"): 1 to 8 discs (ox, oy, r) in the vehicle frame (origin = the pose's
    reference point, x forward, y left; metres), bound to one map set.  Passed as `footprint=` to the validator's checks and to
    HybridAStarBatch.set_footprint; {(0, 0, min_safe_radius)} is the point validator."""

    def __init__(self, map_set, discs):
        self.map = map_set
        self.lib = map_set.lib
        self.discs = [(float(ox), float(oy), float(np.float32(r))) for ox, oy, r in discs]
        arr = (FootprintDisc * max(len(self.discs), 1))()
        for i, (ox, oy, r) in enumerate(self.discs):
            arr[i].ox, arr[i].oy, arr[i].r = ox, oy, r
        h = C.c_void_p()
        check(self.lib.pp_footprint_create(map_set.h, len(self.discs), arr, C.byref(h)))
        self.h = h

    @staticmethod
    def rectangle_discs(length, width, rear_overhang, n_discs):
        """pp_footprint_cover_rectangle: n equal discs on the long axis covering a length x width rectangle whose rear edge lies
        rear_overhang behind the reference point (host arithmetic, no device) -> [(ox, oy, r)]"""
        arr = (FootprintDisc * max(int(n_discs), 1))()
        check(_lib.load().pp_footprint_cover_rectangle(float(length), float(width), float(rear_overhang), int(n_discs), arr))
        return [(arr[i].ox, arr[i].oy, arr[i].r) for i in range(int(n_discs))]

    @classmethod
    def cover_rectangle(cls, map_set, length, width, rear_overhang, n_discs):
        return cls(map_set, cls.rectangle_discs(length, width, rear_overhang, n_discs))

    def close(self):
        if self.h:
            self.lib.pp_footprint_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StateValidatorOccupancyMap:
    """state_validator/state_validator_occupancy_map.{h,cpp}: is_state_valid / is_path_valid, batched.  With `footprint=` a check
    tests the vehicle's discs instead of the reference point against min_safe_radius (class Footprint)."""

    def __init__(self, map_set):
        self.map = map_set
        self.lib = map_set.lib
        self._min_safe_radius = 1.0
        self._min_interp = 0.1
        self._push()

    def _push(self):
        check(self.lib.pp_map_set_validator(self.map.h, C.c_float(self._min_safe_radius), C.c_float(self._min_interp)))

    @property
    def min_safe_radius(self):
        return self._min_safe_radius

    @min_safe_radius.setter
    def min_safe_radius(self, v):
        self._min_safe_radius = float(v)
        self._push()

    @property
    def min_path_interpolation_distance(self):
        return self._min_interp

    @min_path_interpolation_distance.setter
    def min_path_interpolation_distance(self, v):
        self._min_interp = float(v)
        self._push()

    def get_occupancy_map(self):
        return self.map

    def is_state_valid(self, poses, footprint=None, return_clearance=False):
        """poses: (n, 3) array-like -> bool array; or a CUDA float64 tensor -> CUDA uint8 tensor.
        return_clearance (host arrays with a footprint): also min_i (d_i - r_i) as float32, -1 where invalid."""
        if _is_tensor(poses):
            import torch
            n = poses.numel() // 3
            out = torch.empty(n, dtype=torch.uint8, device=poses.device)
            if footprint is not None:
                check(self.lib.pp_check_states_footprint_dev(self.map.h, footprint.h, n, _dev_ptr(poses), _dev_ptr(out)))
            else:
                check(self.lib.pp_check_states_dev(self.map.h, n, _dev_ptr(poses), _dev_ptr(out)))
            return out
        p = _f64(poses, 3)
        out = np.empty(len(p), dtype=np.uint8)
        if footprint is not None:
            clear = np.empty(len(p), dtype=np.float32) if return_clearance else None
            check(self.lib.pp_check_states_footprint(self.map.h, footprint.h, len(p), ptr(p), ptr(out), ptr(clear)))
            return (out.astype(bool), clear) if return_clearance else out.astype(bool)
        if return_clearance:
            raise ValueError("return_clearance needs a footprint")
        check(self.lib.pp_check_states(self.map.h, len(p), ptr(p), ptr(out)))
        return out.astype(bool)

    def is_path_valid(self, start, curvature, length, direction, footprint=None):
        """IsPathValid over constant-steer arcs.  Returns (valid, last_valid_ratio)."""
        s = _f64(start, 3)
        n = len(s)
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(curvature, dtype=np.float64), n))
        ln = np.ascontiguousarray(np.broadcast_to(np.asarray(length, dtype=np.float64), n))
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(direction, dtype=np.int32), n))
        valid = np.empty(n, dtype=np.uint8)
        last = np.empty(n, dtype=np.float32)
        if footprint is not None:
            check(self.lib.pp_check_arcs_footprint(self.map.h, footprint.h, n, ptr(s), ptr(k), ptr(ln), ptr(d), ptr(valid), ptr(last)))
        else:
            check(self.lib.pp_check_arcs(self.map.h, n, ptr(s), ptr(k), ptr(ln), ptr(d), ptr(valid), ptr(last)))
        return valid.astype(bool), last

    def is_segment_valid(self, start_xy, end_xy):
        a = _f64(start_xy, 2)
        b = _f64(end_xy, 2)
        valid = np.empty(len(a), dtype=np.uint8)
        check(self.lib.pp_check_segments(self.map.h, len(a), ptr(a), ptr(b), ptr(valid)))
        return valid.astype(bool)

    def is_rs_path_valid(self, paths, footprint=None):
        """IsPathValid over Reeds-Shepp paths (records of RS_PATH_DTYPE, e.g. from ReedsSheppPaths.connect).  Returns (valid, last)."""
        p = np.ascontiguousarray(paths, dtype=RS_PATH_DTYPE).reshape(-1)
        valid = np.empty(len(p), dtype=np.uint8)
        last = np.empty(len(p), dtype=np.float32)
        if footprint is not None:
            check(self.lib.pp_check_rs_paths_footprint(self.map.h, footprint.h, len(p), ptr(p), ptr(valid), ptr(last)))
        else:
            check(self.lib.pp_check_rs_paths(self.map.h, len(p), ptr(p), ptr(valid), ptr(last)))
        return valid.astype(bool), last

    def is_se2_path_valid(self, start, end, footprint=None):
        """IsPathValid over PathSE2 (paths/path_se2.cpp: linear in position and heading).  Returns (valid, last)."""
        a, b = _f64(start, 3), _f64(end, 3)
        valid = np.empty(len(a), dtype=np.uint8)
        last = np.empty(len(a), dtype=np.float32)
        if footprint is not None:
            check(self.lib.pp_check_se2_paths_footprint(self.map.h, footprint.h, len(a), ptr(a), ptr(b), ptr(valid), ptr(last)))
        else:
            check(self.lib.pp_check_se2_paths(self.map.h, len(a), ptr(a), ptr(b), ptr(valid), ptr(last)))
        return valid.astype(bool), last

    def count_valid_fused(self, n, seed, count_tensor):
        check(self.lib.pp_check_states_fused_dev(self.map.h, int(n), C.c_uint64(seed), _dev_ptr(count_tensor)))


class HybridAStarSearchParameters:
    """HybridAStar::SearchParameters, algo/hybrid_a_star.h:29-50 (same 8-argument constructor order as
    pyplanning.cpp:73-75) plus the two reference-behaviour switches."""

    def __init__(self, min_turning_radius=2.0, direction_switching_cost=0.0, reverse_cost_multiplier=1.0, forward_cost_multiplier=1.0,
                 voronoi_cost_multiplier=1.0, num_generated_motion=5, spatial_resolution=1.0, angular_resolution=0.0872, wheelbase=2.6,
                 heading_alias=True, negative_k_read=True):
        self.wheelbase = wheelbase
        self.min_turning_radius = min_turning_radius
        self.direction_switching_cost = direction_switching_cost
        self.reverse_cost_multiplier = reverse_cost_multiplier
        self.forward_cost_multiplier = forward_cost_multiplier
        self.voronoi_cost_multiplier = voronoi_cost_multiplier
        self.num_generated_motion = num_generated_motion
        self.spatial_resolution = spatial_resolution
        self.angular_resolution = angular_resolution
        self.heading_alias = heading_alias
        self.negative_k_read = negative_k_read

    def to_c(self):
        return HybridParams(self.wheelbase, self.min_turning_radius, self.direction_switching_cost, self.reverse_cost_multiplier,
                            self.forward_cost_multiplier, self.voronoi_cost_multiplier, int(self.num_generated_motion), self.spatial_resolution,
                            self.angular_resolution, int(bool(self.heading_alias)), int(bool(self.negative_k_read)))

    def primitives(self):
        """Steering angles / curvatures / directions in the reference's child order
        (hybrid_a_star.cpp:21-28,65-77; kinematic_bicycle_model.cpp:13-17,34-41)."""
        delta_max = math.atan(self.wheelbase / math.sqrt(math.pow(self.min_turning_radius, 2) - math.pow(0.0, 2)))
        deltas = [0.0]
        for i in range(int(self.num_generated_motion) // 2):
            d = (i + 1) / 2.0 * delta_max
            deltas += [d, -d]
        curv, direc, steer = [], [], []
        for d in deltas:
            tan_s = math.tan(d)
            beta = math.atan(0.0 * tan_s / self.wheelbase)
            k = math.cos(beta) * tan_s / self.wheelbase
            for dr in (0, 1):
                curv.append(k)
                direc.append(dr)
                steer.append(d)
        return np.array(steer), np.array(curv), np.array(direc, dtype=np.int32)


class ReedsSheppSolver:
    """ReedsShepp::Solver::GetOptimalPath, batched (geometry/reeds_shepp.cpp:654-683)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.lib = ctx.lib

    def get_optimal_path(self, start, goal, min_turning_radius, reverse_cost=1.0, forward_cost=1.0, switch_cost=0.0):
        a, b = _f64(start, 3), _f64(goal, 3)
        n = len(a)
        word = np.empty(n, dtype=np.int32)
        tuv = np.empty((n, 3))
        cost = np.empty(n, dtype=np.float32)
        seg = np.empty(n)
        check(self.lib.pp_rs_solve(self.ctx.h, n, ptr(a), ptr(b), C.c_double(min_turning_radius), C.c_float(reverse_cost), C.c_float(forward_cost),
                                   C.c_float(switch_cost), ptr(word), ptr(tuv), ptr(cost), ptr(seg)))
        return word, tuv, cost, seg


class ReedsSheppPaths:
    """PathReedsShepp / PathConnectionReedsShepp as batches of 128-byte records (paths/path_reeds_shepp.{h,cpp}): connect,
    interpolate (+ get_direction), truncate (with the reference's Q11 slot reset), get_cusp_point_ratios -- all on the device."""

    def __init__(self, ctx, min_turning_radius=1.0, direction_switching_cost=0.0, reverse_cost_multiplier=1.0, forward_cost_multiplier=1.0):
        self.ctx, self.lib = ctx, ctx.lib
        self.rmin, self.sw, self.rev, self.fwd = min_turning_radius, direction_switching_cost, reverse_cost_multiplier, forward_cost_multiplier

    def connect(self, start, goal):
        a, b = _f64(start, 3), _f64(goal, 3)
        out = np.zeros(len(a), dtype=RS_PATH_DTYPE)
        check(self.lib.pp_rs_connect(self.ctx.h, len(a), ptr(a), ptr(b), C.c_double(self.rmin), C.c_float(self.rev), C.c_float(self.fwd), C.c_float(self.sw), ptr(out)))
        return out

    def interpolate(self, paths, ratios):
        p = np.ascontiguousarray(paths, dtype=RS_PATH_DTYPE).reshape(-1)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(ratios, dtype=np.float64), len(p)))
        pose = np.empty((len(p), 3))
        direction = np.empty(len(p), dtype=np.int32)
        check(self.lib.pp_rs_path_interpolate(self.ctx.h, len(p), ptr(p), ptr(r), ptr(pose), ptr(direction)))
        return pose, direction

    def truncate(self, paths, ratios, q11=True):
        p = np.ascontiguousarray(paths, dtype=RS_PATH_DTYPE).reshape(-1).copy()
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(ratios, dtype=np.float64), len(p)))
        check(self.lib.pp_rs_path_truncate(self.ctx.h, len(p), ptr(p), ptr(r), int(bool(q11))))
        return p

    def get_cusp_point_ratios(self, paths):
        p = np.ascontiguousarray(paths, dtype=RS_PATH_DTYPE).reshape(-1)
        ratios = np.empty((len(p), 4))
        count = np.empty(len(p), dtype=np.int32)
        check(self.lib.pp_rs_path_cusps(self.ctx.h, len(p), ptr(p), ptr(ratios), ptr(count)))
        return [ratios[i, :count[i]].copy() for i in range(len(p))]


class NonHolonomicHeuristic:
    """NonHolonomicHeuristic::Build (algo/heuristics.cpp:36-76) on the device."""

    @staticmethod
    def build(ctx, lower, upper, params):
        lo = np.ascontiguousarray(lower, dtype=np.float64)
        up = np.ascontiguousarray(upper, dtype=np.float64)
        cp = params.to_c()
        dims = np.zeros(3, dtype=np.int32)
        offs = np.zeros(2)
        check(ctx.lib.pp_nonholo_dims(ptr(lo), ptr(up), C.byref(cp), ptr(dims), ptr(offs)))
        table = np.empty(tuple(int(x) for x in dims))
        check(ctx.lib.pp_nonholo_build(ctx.h, ptr(lo), ptr(up), C.byref(cp), ptr(table)))
        return table, offs


class ObstaclesHeuristic:
    """ObstaclesHeuristic::Update (algo/heuristics.cpp:106-153): one exact-order wavefront per goal."""

    def __init__(self, map_set):
        self.map = map_set
        self.lib = map_set.lib

    def update(self, goals_xy, clearance=0.0):
        """clearance > 0 (include/pp_hip.h, "heuristic clearance"): a cell is also blocked where !(dist >= clearance); 0 is the
        reference's rule."""
        g = _f64(goals_xy, 2)
        out = np.empty((len(g), self.map.rows, self.map.cols), dtype=np.float32)
        if clearance == 0.0:
            check(self.lib.pp_obstacle_heuristic(self.map.h, len(g), ptr(g), ptr(out)))
        else:
            check(self.lib.pp_obstacle_heuristic_clearance(self.map.h, float(clearance), len(g), ptr(g), ptr(out)))
        return out

    def update_dev(self, goals_xy, cost_tensor, clearance=0.0):
        g = _f64(goals_xy, 2)
        if clearance == 0.0:
            check(self.lib.pp_obstacle_heuristic_dev(self.map.h, len(g), ptr(g), _dev_ptr(cost_tensor)))
        else:
            check(self.lib.pp_obstacle_heuristic_clearance_dev(self.map.h, float(clearance), len(g), ptr(g), _dev_ptr(cost_tensor)))

    def clearance_views_build_ms(self, clearance, reps=20):
        """pp_heuristic_clearance_build_ms: mean milliseconds of one build of the clearance's two occupancy views on this map (HIP events)"""
        ms = C.c_float(0.0)
        check(self.lib.pp_heuristic_clearance_build_ms(self.map.h, float(clearance), int(reps), C.byref(ms)))
        return float(ms.value)

    TILE_STATS = ("goals", "tile_visits", "rounds", "candidate_passes", "cells", "handed_over", "wave_cycles", "tiles_per_goal",
                  "cycles_load", "cycles_masks", "cycles_passes", "cycles_requeue", "cycles_store")

    def update_dev_tile_stats(self, goals_xy, cost_tensor):
        """The fields into cost_tensor like update_dev, through the tile form of the wavefront with its work counters:
        returns (dict of TILE_STATS, launch milliseconds)."""
        g = _f64(goals_xy, 2)
        st = np.zeros(16, dtype=np.uint64)
        ms = C.c_float(0.0)
        handed = np.full(len(g), -1, dtype=np.int32)
        check(self.lib.pp_obstacle_heuristic_tiles_stats(self.map.h, len(g), ptr(g), _dev_ptr(cost_tensor), ptr(st), C.byref(ms), ptr(handed)))
        d = dict(zip(self.TILE_STATS, (int(x) for x in st)))
        d["handed_over_goals"] = sorted(int(x) for x in handed[:d["handed_over"]])
        return d, float(ms.value)


class Tree:
    """Tree::GetNearestNodes (utils/tree.h:73-116): exact kNN, squared L2, ascending."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.lib = ctx.lib

    def get_nearest_nodes(self, points_xy, queries_xy, k=1):
        p, q = _f64(points_xy, 2), _f64(queries_xy, 2)
        idx = np.empty((len(q), k), dtype=np.int32)
        d2 = np.empty((len(q), k))
        check(self.lib.pp_knn(self.ctx.h, len(p), ptr(p), len(q), ptr(q), int(k), ptr(idx), ptr(d2)))
        return idx, d2


class HybridAStarBatch:
    """HybridAStar graph search for batches of independent (start, goal, seed) queries.

    Single-query use mirrors PathPlannerSE2Base (pyplanning.cpp:66-71):
        planner.set_init_state(pose); planner.set_goal_state(pose); planner.search_path(); planner.get_path()
    """

    def __init__(self, validator, params=None, max_batch=1, max_nodes=16384, search_rows=0):
        """search_rows: rows (= node/heap/key-map buffer sets) of the four-queries-per-wave search kernel that
        throughput-sized planners (max_batch > 64) use; 0 = as many as can be resident.  Pass resident rows / k when k
        planners share one GPU."""
        self.validator = validator
        self.map = validator.map
        self.lib = self.map.lib
        self.params = params if params is not None else HybridAStarSearchParameters()
        self.cparams = self.params.to_c()
        self.max_batch, self.max_nodes = int(max_batch), int(max_nodes)
        h = C.c_void_p()
        check(self.lib.pp_planner_create_ex(self.map.h, C.byref(self.cparams), self.max_batch, self.max_nodes, int(search_rows), C.byref(h)))
        self.h = h
        self.num_primitives = self.lib.pp_planner_num_primitives(self.h)
        self.search_rows = self.lib.pp_planner_search_rows(self.h)  # 0: one-query-per-wave kernel
        self._init = np.zeros(3)
        self._goal = np.zeros(3)
        self._seed = 0
        self._results = None
        self.footprint = None  # set_footprint
        self.is_initialized = False

    def set_primitives(self, steering_angles):
        """Explicit steering-angle list instead of the one hybrid_a_star.cpp:21-28 generates (P = 2 * len: forward + backward each)."""
        d = np.ascontiguousarray(steering_angles, dtype=np.float64)
        check(self.lib.pp_planner_set_primitives(self.h, len(d), ptr(d)))
        self.num_primitives = self.lib.pp_planner_num_primitives(self.h)

    def set_footprint(self, footprint):
        """Every validity question of the search (start pose, child poses, arc marches and their truncation, the analytic expansion)
        goes through `footprint` (class Footprint) instead of the point validator; None restores the point validator.  Planners of the
        one-query-per-wave kernel only (max_batch <= 64, or PP_SEARCH_ROWS=0 in the environment): others raise PPError."""
        check(self.lib.pp_planner_set_footprint(self.h, footprint.h if footprint is not None else None))
        self.footprint = footprint  # (keeps it alive on this side too)

    def set_heuristic_clearance(self, radius):
        """Heuristic clearance (include/pp_hip.h): for the obstacle-heuristic fields of every later batch a cell is blocked iff it is
        occupied or !(dist >= radius); the search itself is untouched.  0 (the default) is the reference's rule.  radius <= the
        validator's min_safe_radius keeps the heuristic a lower bound; a larger one is the caller's choice."""
        check(self.lib.pp_planner_set_heuristic_clearance(self.h, float(radius)))

    @property
    def heuristic_clearance(self):
        r = C.c_float(0.0)
        check(self.lib.pp_planner_heuristic_clearance(self.h, C.byref(r)))
        return float(r.value)

    def initialize(self, nonholo_table=None):
        """HybridAStar::Initialize (hybrid_a_star.cpp:206-235): builds the non-holonomic table on the
        device unless one is supplied."""
        if nonholo_table is not None:
            t = np.ascontiguousarray(nonholo_table, dtype=np.float64)
            check(self.lib.pp_planner_set_nonholo_table(self.h, ptr(t)))
        else:
            check(self.lib.pp_planner_set_nonholo_table(self.h, None))
        self.is_initialized = True
        return True

    def nonholo_table(self):
        cp = self.cparams
        dims = np.zeros(3, dtype=np.int32)
        offs = np.zeros(2)
        lo = np.ascontiguousarray(self.map.lower)
        up = np.ascontiguousarray(self.map.upper)
        check(self.lib.pp_nonholo_dims(ptr(lo), ptr(up), C.byref(cp), ptr(dims), ptr(offs)))
        t = np.empty(tuple(int(x) for x in dims))
        check(self.lib.pp_planner_get_nonholo_table(self.h, ptr(t)))
        return t

    # -- batch API --------------------------------------------------------
    def search_batch(self, starts, goals, seeds):
        if not self.is_initialized:
            # hybrid_a_star.cpp:243-246: "The algorithm has not been initialized successfully."
            return None
        s, g = _f64(starts, 3), _f64(goals, 3)
        sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        n = len(s)
        res = (QueryResult * n)()
        check(self.lib.pp_planner_search_batch(self.h, n, ptr(s), ptr(g), ptr(sd), C.cast(res, C.c_void_p)))
        self._results = res
        self._n = n
        return res

    def start_after_fields_of(self, predecessor):
        """the next batch of this planner starts on the device once `predecessor`'s current batch has its heuristic fields (one-shot):
        phases the batches in flight one wavefront apart instead of letting them run in step (scheduling only)"""
        check(self.lib.pp_planner_start_after_fields_of(self.h, predecessor.h))

    def search_batch_dev(self, starts_t, goals_t, seeds_t):
        n = starts_t.numel() // 3
        check(self.lib.pp_planner_search_batch_dev(self.h, n, _dev_ptr(starts_t), _dev_ptr(goals_t), _dev_ptr(seeds_t)))
        self._n = n

    def fetch_results(self, n=None):
        n = self._n if n is None else n
        res = (QueryResult * n)()
        check(self.lib.pp_planner_fetch_results(self.h, n, C.cast(res, C.c_void_p)))
        self._results = res
        return res

    def last_timings(self):
        a, b = C.c_float(), C.c_float()
        check(self.lib.pp_planner_last_timings(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def get_path_of(self, q):
        r = self._results[q]
        n = r.n_path
        poses = np.empty((n, 3))
        kind = np.empty(n, dtype=np.int32)
        prim = np.empty(n, dtype=np.int32)
        length = np.empty(n)
        tuv = np.empty((n, 3))
        if n:
            check(self.lib.pp_planner_get_path(self.h, q, ptr(poses), ptr(kind), ptr(prim), ptr(length), ptr(tuv)))
        return dict(poses=poses, kind=kind, prim=prim, length=length, tuv=tuv)

    def postprocess(self, n_queries=None, path_interpolation=0.1, smoother=None, max_points=2048):
        """HybridAStar::SearchPath's post-processing (hybrid_a_star.cpp:260-304) for the first n queries of the last batch: composite
        path, sampling every `path_interpolation` metres with cusp snapping, Smoother::Smooth.  `smoother`: dict of
        Smoother::Parameters fields to override (defaults: smoother.h:28-60, max_curvature = 1 / min_turning_radius).
        Returns one PostResult per query (n_points, smoothing_status, iterations, length)."""
        n = len(self._results) if n_queries is None else int(n_queries)
        sp = _smoother_params(smoother, self.params)
        out = (PostResult * max(n, 1))()
        check(self.lib.pp_planner_postprocess(self.h, n, C.c_float(path_interpolation), C.byref(sp) if sp is not None else None, int(max_points), out))
        self._post = list(out)[:n]
        return self._post

    def get_processed_path(self, q):
        """sampled path, cusp flags and smoothed path of query q; `path` = what HybridAStar::GetPath() returns (the smoothed path
        when smoothing succeeded, else the sampled one, hybrid_a_star.cpp:293-303)"""
        r = self._post[q]
        n = r.n_points
        sampled, smoothed = np.empty((n, 3)), np.empty((n, 3))
        cusp = np.empty(n, dtype=np.uint8)
        if n:
            check(self.lib.pp_planner_get_processed_path(self.h, q, ptr(sampled), ptr(cusp), ptr(smoothed)))
        return _processed_path(r, sampled, cusp, smoothed)

    def revalidate(self, n_queries=None, map_set=None):
        """Are the plans of the first n queries of the last batch still collision-free on `map_set` (an OccupancyMapSet of the same
        context; None: the planner's own map) as it is now (pp_planner_revalidate)?  Every edge is marched as the search marched it, with
        the planner's footprint if it has one, then the last pose gets the state check.  Returns one RevalidateResult per query
        (status, n_edges, blocked_edge, blocked_ratio, valid_length, length)."""
        n = len(self._results) if n_queries is None else int(n_queries)
        out = (RevalidateResult * max(n, 1))()
        check(self.lib.pp_planner_revalidate(self.h, map_set.h if map_set is not None else None, n, out))
        return list(out)[:n]

    def stamp(self, n_queries=None, map_set=None, values=None, from_length=None, to_length=None, spacing=0.1, margin=0.0):
        """Stamps the plans of the first n queries of the last batch into the int32 occupancy grid of `map_set` (None: the planner's own
        map): pp_planner_stamp, the batch form of HybridAStarPipeline.stamp, with the planner's footprint if it has one.  Returns one
        StampResult per query."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _stamp(n, values, from_length, to_length, spacing, margin,
                      lambda v, a, b, sp, out: self.lib.pp_planner_stamp(self.h, map_set.h if map_set is not None else None, n, ptr(v), ptr(a), ptr(b), C.byref(sp), out))

    def locate(self, poses, n_queries=None, from_length=None, to_length=None, spacing=0.1, heading_weight=0.0):
        """Locates the vehicle poses `poses` [n, 3] on the plans of the first n queries of the last batch: pp_planner_locate, the batch form of
        HybridAStarPipeline.locate.  Returns one LocateResult per query."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _locate(n, poses, from_length, to_length, spacing, heading_weight,
                       lambda v, a, b, lp, out: self.lib.pp_planner_locate(self.h, n, ptr(v), ptr(a), ptr(b), C.byref(lp), out))

    def speed_profile(self, n_queries=None, map_set=None, from_length=None, to_length=None, v_start=None, v_end=None, max_samples=2048, samples=True, **limits):
        """Speeds and arrival times along the plans of the first n queries of the last batch: pp_planner_speed_profile, the batch form of
        HybridAStarPipeline.speed_profile, with the same arguments and return value."""
        n = len(self._results) if n_queries is None else int(n_queries)
        self._profiled = None
        out = _speed_profile(n, from_length, to_length, v_start, v_end, max_samples, samples, limits,
                             lambda a, b, vs, ve, sp, rows, out: self.lib.pp_planner_speed_profile(self.h, map_set.h if map_set is not None else None, n, ptr(a), ptr(b), ptr(vs),
                                                                                                   ptr(ve), C.byref(sp), int(max_samples), ptr(rows), out))
        self._profiled = _profiled(range(n), out[0] if samples else out, max_samples)
        return out

    def conflicts(self, t_start, n_queries=None, pairs=None, t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False, hold_after=False, poses=False):
        """Space-time conflicts between the plans of the first n queries of the last batch on the timetables of the planner's last speed_profile call:
        pp_planner_conflicts, the batch form of HybridAStarPipeline.conflicts, with the same arguments (pair indices are query indices) and return value."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _conflicts(n, t_start, pairs, t_from, t_to, dt, margin, hold_before, hold_after, poses,
                          lambda ts, npairs, pr, cp, xyt, plans, out: self.lib.pp_planner_conflicts(self.h, n, ptr(ts), npairs, ptr(pr), C.byref(cp), ptr(xyt), plans, out))

    def deconflict(self, t_start, n_queries=None, pairs=None, t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False, hold_after=False, max_delay_steps=0):
        """Start delays that clear the conflicts between the plans of the first n queries of the last batch, by priority (the query index):
        pp_planner_deconflict, the batch form of HybridAStarPipeline.deconflict, with the same arguments (pair indices are query indices) and return value."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _deconflict(n, t_start, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps,
                           lambda ts, npairs, pr, dp, out: self.lib.pp_planner_deconflict(self.h, n, ptr(ts), npairs, ptr(pr), C.byref(dp), ptr(out)))

    def deconflict_waits(self, t_start, n_queries=None, pairs=None, no_start_wait=None, fixed=None, t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False,
                         hold_after=False, max_delay_steps=0, max_places=0, places=False):
        """Waits at the start or at a timetable's stops that clear the conflicts between the plans of the first n queries of the last batch, by priority
        (the query index): pp_planner_deconflict_waits, the batch form of HybridAStarPipeline.deconflict_waits, with the same arguments (pair indices
        are query indices) and return value."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _deconflict_waits(n, t_start, no_start_wait, fixed, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps, max_places, places,
                                 lambda ts, flags, fx, npairs, pr, wp, counts, listed, out: self.lib.pp_planner_deconflict_waits(
                                     self.h, n, ptr(ts), ptr(flags), ptr(fx), npairs, ptr(pr), C.byref(wp), ptr(counts), ptr(listed), ptr(out)))

    def deconflict_tracks(self, t_start, tracks, n_queries=None, pairs=None, t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False, hold_after=False, max_delay_steps=0,
                          details=True):
        """Start delays that clear the conflicts between the plans of the first n queries of the last batch and with the tracked movers `tracks`:
        pp_planner_deconflict_tracks, the batch form of HybridAStarPipeline.deconflict_tracks, with the same arguments (pair indices are query indices) and
        return value."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _deconflict_tracks(n, t_start, tracks, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps, details,
                                  lambda ts, npairs, pr, dp, tk, out, rec: self.lib.pp_planner_deconflict_tracks(self.h, n, ptr(ts), npairs, ptr(pr), C.byref(dp), tk, ptr(out),
                                                                                                                 ptr(rec)))

    def candidate_pairs(self, t_start, n_queries=None, times_per_box=64, max_delay_steps=0, boxes=False, max_pairs=None, **lattice):
        """The pairs of the plans of the first n queries of the last batch that can meet: pp_planner_candidate_pairs, the batch form of
        HybridAStarPipeline.candidate_pairs, with the same arguments (pair indices are query indices) and return value."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _candidate_pairs(n, t_start, times_per_box, max_delay_steps, boxes, max_pairs, lattice,
                                lambda ts, pp, pr, fb, bx, sm: self.lib.pp_planner_candidate_pairs(self.h, n, ptr(ts), C.byref(pp), ptr(pr), ptr(fb), ptr(bx), C.byref(sm)))

    def timetable(self, values, n_queries=None, by="length", max_stops=16):
        """Look-ups into the timetables of the first n queries of the last batch and the lists of their stops: pp_planner_timetable, the batch form of
        HybridAStarPipeline.timetable, with the same arguments and return value."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _timetable(n, values, by, max_stops, lambda P, v, tp, pl, st, out: self.lib.pp_planner_timetable(self.h, n, P, ptr(v), C.byref(tp), ptr(pl), ptr(st), ptr(out)))

    def retime(self, holds, n_queries=None, rows=False):
        """Holds written into the timetables of the first n queries of the last batch: pp_planner_retime, the batch form of HybridAStarPipeline.retime,
        with the same arguments (a hold's plan is a query index) and return value."""
        n = len(self._results) if n_queries is None else int(n_queries)
        return _retime(n, range(n), getattr(self, "_profiled", None), holds, rows,
                       lambda H, hd, buf, out: self.lib.pp_planner_retime(self.h, n, H, ptr(hd), ptr(buf), ptr(out)))

    def certify_lattice(self, q):
        """SURVEY 7.3 H2 as a contract (pp_planner_certify_lattice): created nodes and logged lattice-line children of query q recomputed on
        the host with glibc; returns (checked, cell mismatches, unverified events, largest pose difference).  mismatches == unverified == 0
        certifies the query's discrete outputs.  One-query-per-wave planners only."""
        a, b, c, d = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_double(0)
        check(self.lib.pp_planner_certify_lattice(self.h, int(q), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def get_expanded_of(self, q):
        r = self._results[q]
        cells = np.empty((r.n_expanded, 3), dtype=np.int32)
        if r.n_expanded:
            check(self.lib.pp_planner_get_expanded(self.h, q, ptr(cells)))
        return cells

    def get_obstacle_field_of(self, q):
        """the obstacle-heuristic field query q of the last batch was searched with: [rows, cols] float32, +inf where unexplored"""
        out = np.empty((self.map.rows, self.map.cols), dtype=np.float32)
        check(self.lib.pp_planner_get_obstacle_field(self.h, int(q), ptr(out)))
        return out

    # -- PathPlannerSE2Base-shaped single query ---------------------------
    def set_init_state(self, pose):
        self._init = np.asarray(pose, dtype=np.float64)

    def set_goal_state(self, pose):
        self._goal = np.asarray(pose, dtype=np.float64)

    def set_seed(self, seed):
        self._seed = int(seed)

    def search_path(self):
        res = self.search_batch([self._init], [self._goal], [self._seed])
        if res is None:
            return Status.FAILURE
        return Status.SUCCESS if res[0].status == 0 else Status.FAILURE

    def get_path(self):
        """Graph-search path nodes (GetPath of the A* layer); post-processing/smoothing is out of scope."""
        if self._results is None:
            return np.empty((0, 3))
        return self.get_path_of(0)["poses"]

    def get_graph_search_optimal_cost(self):
        return self._results[0].cost if self._results is not None else float("inf")

    def close(self):
        if self.h:
            self.lib.pp_planner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HybridAStarPipeline:
    """Streaming form of the batched planner (include/pp_hip.h: pp_pipeline_*): queries are submitted as they come, every goal's
    obstacle-heuristic field is handed by the wavefront kernel to ONE persistent search grid through a device-side queue, results are
    polled in completion order and their field slots recycled.  Per-query results are those of HybridAStarBatch.search_batch."""

    def __init__(self, validator, params=None, capacity=4096, max_nodes=81920, search_rows=0, log_expansions=False):
        self.validator = validator
        self.map = validator.map
        self.lib = self.map.lib
        self.params = params if params is not None else HybridAStarSearchParameters()
        self.cparams = self.params.to_c()
        h = C.c_void_p()
        check(self.lib.pp_pipeline_create(self.map.h, C.byref(self.cparams), int(capacity), int(max_nodes), int(search_rows), int(bool(log_expansions)), C.byref(h)))
        self.h = h
        self.planner_h = C.c_void_p(self.lib.pp_pipeline_planner(self.h))
        self.capacity = self.lib.pp_pipeline_capacity(self.h)
        self.search_rows = self.lib.pp_pipeline_search_rows(self.h)
        self.num_primitives = self.lib.pp_planner_num_primitives(self.planner_h)
        self._held = {}  # ticket -> QueryResult of completed queries polled with release=False
        self._footprint = None  # set_footprint

    def set_footprint(self, footprint):
        """Every validity question of the pipeline's search grid goes through `footprint` (class Footprint; see HybridAStarBatch.set_footprint)
        instead of the point validator; None restores the point validator, and the grid then runs the kernel it ran before.  The grid's waves
        keep the footprint they were launched with, so the call raises PPError ("in flight") unless every submitted query has been polled;
        an accepted call waits for the old grid's waves.  The pipeline holds its own reference: the Footprint object may be closed afterwards."""
        check(self.lib.pp_pipeline_set_footprint(self.h, footprint.h if footprint is not None else None))
        self._footprint = footprint

    @property
    def footprint(self):
        """the Footprint last accepted by set_footprint, or None"""
        return self._footprint

    def set_heuristic_clearance(self, radius):
        """Heuristic clearance of the fields of every goal submitted afterwards (see HybridAStarBatch.set_heuristic_clearance).  Fields
        already built belong to the old rule, so the call raises PPError ("in flight") unless every submitted query has been polled."""
        check(self.lib.pp_pipeline_set_heuristic_clearance(self.h, float(radius)))

    @property
    def heuristic_clearance(self):
        r = C.c_float(0.0)
        check(self.lib.pp_pipeline_heuristic_clearance(self.h, C.byref(r)))
        return float(r.value)

    def initialize(self, nonholo_table=None):
        t = None if nonholo_table is None else np.ascontiguousarray(nonholo_table, dtype=np.float64)
        check(self.lib.pp_planner_set_nonholo_table(self.planner_h, ptr(t) if t is not None else None))
        return True

    def nonholo_table(self):
        cp = self.cparams
        dims = np.zeros(3, dtype=np.int32)
        offs = np.zeros(2)
        lo, up = np.ascontiguousarray(self.map.lower), np.ascontiguousarray(self.map.upper)
        check(self.lib.pp_nonholo_dims(ptr(lo), ptr(up), C.byref(cp), ptr(dims), ptr(offs)))
        t = np.empty(tuple(int(x) for x in dims))
        check(self.lib.pp_planner_get_nonholo_table(self.planner_h, ptr(t)))
        return t

    def submit(self, starts, goals, seeds):
        """Returns the tickets of the queries taken (a prefix of the input: as many as there were free slots)."""
        s, g = _f64(starts, 3), _f64(goals, 3)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        n = len(s)
        tickets = np.empty(n, dtype=np.uint64)
        k = C.c_int32(0)
        check(self.lib.pp_pipeline_submit(self.h, n, ptr(s), ptr(g), ptr(sd), ptr(tickets), C.byref(k)))
        return tickets[:k.value]

    def submit_dev(self, starts_t, goals_t, seeds_t, n=None, offset=0):
        """device tensors ([n, 3] f64, [n, 3] f64, [n] int64 / uint64); returns (first ticket, number taken)"""
        n = starts_t.numel() // 3 - offset if n is None else n
        tickets = np.empty(max(n, 1), dtype=np.uint64)
        k = C.c_int32(0)
        check(self.lib.pp_pipeline_submit_dev(self.h, n, C.c_void_p(starts_t.data_ptr() + 24 * offset), C.c_void_p(goals_t.data_ptr() + 24 * offset),
                                              C.c_void_p(seeds_t.data_ptr() + 8 * offset), ptr(tickets), C.byref(k)))
        return (int(tickets[0]) if k.value else -1), k.value

    def poll(self, max_results=4096, release=True):
        """Completed queries so far: (tickets [k] uint64, results [k] QueryResult); never blocks."""
        tickets = np.empty(max_results, dtype=np.uint64)
        res = (QueryResult * max_results)()
        k = C.c_int32(0)
        check(self.lib.pp_pipeline_poll(self.h, int(max_results), ptr(tickets), C.cast(res, C.c_void_p), int(bool(release)), C.byref(k)))
        if not release:
            for i in range(k.value):
                self._held[int(tickets[i])] = res[i]
        return tickets[:k.value], res

    def poll_array(self, max_results=4096):
        """poll(release=True) as numpy arrays: (tickets [k] uint64, results [k] of _lib.QUERY_RESULT_DTYPE)"""
        from ._lib import QUERY_RESULT_DTYPE
        tickets = np.empty(max_results, dtype=np.uint64)
        res = np.empty(max_results, dtype=QUERY_RESULT_DTYPE)
        k = C.c_int32(0)
        check(self.lib.pp_pipeline_poll(self.h, int(max_results), ptr(tickets), ptr(res), 1, C.byref(k)))
        return tickets[:k.value], res[:k.value]

    def poll_array_held(self, max_results=4096):
        """poll(release=False) as numpy arrays: the slots stay held until get_paths(..., release=True) / release(); for callers that fetch
        every plan (bench.py)"""
        from ._lib import QUERY_RESULT_DTYPE
        tickets = np.empty(max_results, dtype=np.uint64)
        res = np.empty(max_results, dtype=QUERY_RESULT_DTYPE)
        k = C.c_int32(0)
        check(self.lib.pp_pipeline_poll(self.h, int(max_results), ptr(tickets), ptr(res), 0, C.byref(k)))
        return tickets[:k.value], res[:k.value]

    def get_paths(self, tickets, max_poses=256, release=True, out=None, n_out=None):
        """GetGraphSearchPath of completed, held queries, start pose first (pp_pipeline_get_paths): returns (poses [k, max_poses, 3] f64,
        n_poses [k] int32); rows beyond n_poses[i] are unspecified.  The poses arrive in pinned host memory with the completion records:
        this is a host copy."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        k = len(t)
        poses = out if out is not None else np.empty((max(k, 1), max_poses, 3))
        n_poses = n_out if n_out is not None else np.zeros(max(k, 1), dtype=np.int32)
        assert poses.flags.c_contiguous and poses.shape[0] >= k and poses.shape[1] == max_poses
        check(self.lib.pp_pipeline_get_paths(self.h, k, ptr(t), int(max_poses), ptr(poses), ptr(n_poses), int(bool(release))))
        if release:
            for x in t:
                self._held.pop(int(x), None)
                getattr(self, "_post_by_ticket", {}).pop(int(x), None)
        return poses[:k], n_poses[:k]

    def backlog(self):
        """(ready, searching): queries whose field is built and waiting for a row / claimed by a row, as of the last poll"""
        a, b = C.c_int64(0), C.c_int64(0)
        check(self.lib.pp_pipeline_backlog(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def timings(self):
        """kernel launch durations since the last call (pp_pipeline_timings), as a dict"""
        a, d, f = C.c_double(), C.c_double(), C.c_double()
        b, c, e = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib.pp_pipeline_timings(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e), C.byref(f)))
        return dict(wavefront_ms_total=a.value, wavefront_launches=b.value, wavefront_goals=c.value, search_ms_total=d.value, search_launches=e.value, search_max_ms=f.value)

    def in_flight(self):
        return self.lib.pp_pipeline_in_flight(self.h)

    def alive_waves(self):
        """diagnostics: waves of the search grid that own their index right now (blocking copy)"""
        return self.lib.pp_pipeline_alive_waves(self.h)

    def free_slots(self):
        return self.lib.pp_pipeline_free_slots(self.h)

    def release(self, tickets):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        check(self.lib.pp_pipeline_release(self.h, len(t), ptr(t)))
        for x in t:
            self._held.pop(int(x), None)
            getattr(self, "_post_by_ticket", {}).pop(int(x), None)

    def get_path_of(self, ticket):
        """solution path of a completed query polled with release=False"""
        slot = self.lib.pp_pipeline_slot_of(self.h, C.c_uint64(int(ticket)))
        if slot < 0:
            raise ValueError("ticket is not a completed, held query")
        n = self._held[int(ticket)].n_path
        poses, kind, prim, length, tuv = np.empty((n, 3)), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n), np.empty((n, 3))
        if n:
            check(self.lib.pp_planner_get_path(self.planner_h, slot, ptr(poses), ptr(kind), ptr(prim), ptr(length), ptr(tuv)))
        return dict(poses=poses, kind=kind, prim=prim, length=length, tuv=tuv)

    def postprocess_held(self, n_slots=None, path_interpolation=0.1, smoother=None, max_points=2048):
        """HybridAStar::SearchPath's post-processing (hybrid_a_star.cpp:260-304) over the field slots 0 .. n_slots-1 of the pipeline's buffer
        set (pp_planner_postprocess on pp_pipeline_planner()): meaningful for slots whose queries are completed and HELD (polled with
        release=False); read a query's processed path with get_processed_path_of(ticket).  The smoother knows the point validator only:
        with a footprint set (set_footprint) the search's plans respect it, the smoothed paths are checked against the reference point alone.
        postprocess(tickets) is the form by ticket: it works on the held queries named, with buffers sized by the call, may run with
        queries in flight, and checks the smoothed samples against the footprint."""
        n = self.capacity if n_slots is None else int(n_slots)
        sp = _smoother_params(smoother, self.params)
        out = (PostResult * max(n, 1))()
        check(self.lib.pp_planner_postprocess(self.planner_h, n, C.c_float(path_interpolation), C.byref(sp) if sp is not None else None, int(max_points), out))
        self._post = list(out)[:n]
        return self._post

    def get_processed_path_of(self, ticket):
        slot = self.lib.pp_pipeline_slot_of(self.h, C.c_uint64(int(ticket)))
        if slot < 0:
            raise ValueError("ticket is not a completed, held query")
        r = self._post[slot]
        n = r.n_points
        sampled, smoothed = np.empty((n, 3)), np.empty((n, 3))
        cusp = np.empty(n, dtype=np.uint8)
        if n:
            check(self.lib.pp_planner_get_processed_path(self.planner_h, slot, ptr(sampled), ptr(cusp), ptr(smoothed)))
        return _processed_path(r, sampled, cusp, smoothed)

    def postprocess(self, tickets, path_interpolation=0.1, smoother=None, max_points=2048):
        """HybridAStar::SearchPath's post-processing (hybrid_a_star.cpp:260-304) of the completed, HELD queries `tickets`
        (pp_pipeline_postprocess), in that order; legal while other queries are in flight.  `smoother` as HybridAStarBatch.postprocess.
        Returns one PostResult per ticket.  With a footprint set (set_footprint) a path the smoother kept is checked sample by sample
        against it: smoothing_status -2 when one fails, and the sampled path is then the result.  Raises PPError, with nothing launched,
        for a ticket that is unknown, released, in flight or given twice."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        sp = _smoother_params(smoother, self.params)
        out = (PostResult * max(len(t), 1))()
        check(self.lib.pp_pipeline_postprocess(self.h, len(t), ptr(t), C.c_float(path_interpolation), C.byref(sp) if sp is not None else None, int(max_points), out))
        self._post_by_ticket = {int(x): out[i] for i, x in enumerate(t)}
        self._post_points = int(max_points)
        return list(out)[:len(t)]

    def get_processed_paths(self, tickets, release=False):
        """Sampled path, cusp flags and smoothed path of tickets of the LAST postprocess() call that are still held
        (pp_pipeline_get_processed_paths): a list of dicts shaped like get_processed_path_of's; `path` = what HybridAStar::GetPath()
        returns (the smoothed path when status >= 0, else the sampled one).  Any other ticket raises PPError."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        k = len(t)
        post = getattr(self, "_post_by_ticket", {})
        cap = max([post[int(x)].n_points for x in t if int(x) in post] + [1])
        sampled, smoothed = np.empty((max(k, 1), cap, 3)), np.empty((max(k, 1), cap, 3))
        cusp = np.empty((max(k, 1), cap), dtype=np.uint8)
        n_points = np.zeros(max(k, 1), dtype=np.int32)
        check(self.lib.pp_pipeline_get_processed_paths(self.h, k, ptr(t), cap, ptr(sampled), ptr(cusp), ptr(smoothed), ptr(n_points), int(bool(release))))
        out = []
        for i, x in enumerate(t):
            r, n = post[int(x)], int(n_points[i])
            out.append(_processed_path(r, sampled[i, :n].copy(), cusp[i, :n], smoothed[i, :n].copy()))
        if release:
            for x in t:
                self._held.pop(int(x), None)
                post.pop(int(x), None)
        return out

    def revalidate(self, tickets, map_set=None):
        """Are the plans of the completed, HELD queries `tickets` still collision-free on `map_set` (an OccupancyMapSet of the same
        context, any geometry; None: the pipeline's own map) as it is NOW (pp_pipeline_revalidate)?  Legal while other queries are in
        flight.  Every edge is marched as the search marched it -- with the pipeline's footprint if one is set, else the point validator with
        the target map's tunables -- then the last pose gets the state check.  Returns one RevalidateResult per ticket, in that order:
        status 0 valid, 1 blocked at `blocked_edge` (root first, from 1) after `blocked_ratio` of it, 2 only the goal pose fails, -1 no
        plan; valid_length = metres drivable from the start.  The results of the last postprocess() call stay readable.  Raises PPError,
        with nothing launched, for a ticket that is unknown, released, in flight or given twice."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        out = (RevalidateResult * max(len(t), 1))()
        check(self.lib.pp_pipeline_revalidate(self.h, map_set.h if map_set is not None else None, len(t), ptr(t), out))
        return list(out)[:len(t)]

    def stamp(self, tickets, map_set=None, values=None, from_length=None, to_length=None, spacing=0.1, margin=0.0):
        """Stamps the plans of the completed, HELD queries `tickets` into the int32 occupancy grid of `map_set` (an OccupancyMapSet of the
        same context, any geometry; None: the pipeline's own map, refused with queries in flight): pp_pipeline_stamp, whose definition is in
        include/pp_hip.h.  Every cell whose centre lies within r_i + margin of disc i's centre at a sample pose becomes max(cell, values[k]);
        the samples lie every `spacing` metres along each edge (both ends included) inside [from_length[k], to_length[k]] metres from the
        start (None: the whole plan).  The discs are the pipeline's footprint, else (0, 0, min_safe_radius) of the pipeline's own map.
        Stamping another map than the pipeline's own is legal while other queries are in flight.  The target's distance fields are NOT
        rebuilt: run update_gvd on it when they are to follow.  Returns one StampResult per ticket (status, n_samples, cell_box, length).
        Raises PPError, with nothing launched or written, for a ticket that is unknown, released, in flight or given twice, a negative
        value, a NaN in a window, a spacing that is not > 0 or a margin that is not >= 0."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _stamp(len(t), values, from_length, to_length, spacing, margin,
                      lambda v, a, b, sp, out: self.lib.pp_pipeline_stamp(self.h, map_set.h if map_set is not None else None, len(t), ptr(t), ptr(v), ptr(a), ptr(b), C.byref(sp), out))

    def locate(self, tickets, poses, from_length=None, to_length=None, spacing=0.1, heading_weight=0.0):
        """Where is vehicle k, at pose poses[k] = (x, y, theta), on the plan of the completed, HELD query tickets[k]?  pp_pipeline_locate, whose
        definition is in include/pp_hip.h: the point of the plan closest to the vehicle under the cost (ex^2 + ey^2) + (heading_weight * dtheta)^2,
        searched over the samples every `spacing` metres along each edge (the stamp's schedule) inside [from_length[k], to_length[k]] metres from the
        start (None: the whole plan), then over the lattice i * spacing / 32 around the best sample.  heading_weight > 0 (metres per radian) chooses
        between the branches of a cusp or a self-crossing; so does a window.  No map is read and nothing but the records is written: legal while
        other queries are in flight.  Returns one LocateResult per ticket (status, edge, direction, n_samples, s, ratio, distance, along, lateral,
        heading_error, length, pose); r.s is what stamp's from_length takes and what revalidate's valid_length is read against.
        Raises PPError, with nothing launched, for a ticket that is unknown, released, in flight or given twice, a pose that is not finite, a NaN
        in a window, a spacing that is not > 0 or a heading_weight that is not >= 0."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _locate(len(t), poses, from_length, to_length, spacing, heading_weight,
                       lambda v, a, b, lp, out: self.lib.pp_pipeline_locate(self.h, len(t), ptr(t), ptr(v), ptr(a), ptr(b), C.byref(lp), out))

    def speed_profile(self, tickets, map_set=None, from_length=None, to_length=None, v_start=None, v_end=None, max_samples=2048, samples=True, **limits):
        """How fast may the vehicle of the completed, HELD query tickets[k] drive along its plan, and when is it where?  pp_pipeline_speed_profile, whose
        definition is in include/pp_hip.h: at every sample of the stamp's schedule (`spacing`) inside [from_length[k], to_length[k]] metres from the start
        (None: the whole plan) the speed under v_max_forward / v_max_reverse, the lateral limit v^2 kappa <= a_lat, the acceleration limits a_acc / a_dec, a
        stop (plus `dwell` seconds) at every change of travel direction, v_start[k] at the first and v_end[k] at the last sample (None: 0) and, with
        clearance_gain > 0, v <= v_floor + clearance_gain * clearance on map_set (None: the pipeline's own map); and the arrival time.  `limits` are the
        fields of SpeedProfileParams (defaults: spacing 0.1, v_max_forward 5, v_max_reverse 2, a_acc 1.5, a_dec 2.5, a_lat 2, dwell 0, clearance_gain 0,
        v_floor 0).  Nothing but the call's own buffers is written: legal while other queries are in flight.
        Returns the SpeedProfileResult records and, with samples=True, a list of (n_samples, 3) arrays of (s, v, t), empty for a plan whose status is
        not 0 (status -5: more than max_samples samples).  r.s of a locate result is what from_length takes.
        Raises PPError, with nothing launched, for a ticket that is unknown, released, in flight or given twice, a limit outside its domain,
        max_samples < 1, a NaN in a window, a v_start / v_end that is not finite and >= 0, a foreign map, or a map without a distance grid when
        clearance_gain > 0."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        self._profiled = None
        out = _speed_profile(len(t), from_length, to_length, v_start, v_end, max_samples, samples, limits,
                             lambda a, b, vs, ve, sp, rows, out: self.lib.pp_pipeline_speed_profile(self.h, map_set.h if map_set is not None else None, len(t), ptr(t), ptr(a),
                                                                                                    ptr(b), ptr(vs), ptr(ve), C.byref(sp), int(max_samples), ptr(rows), out))
        self._profiled = _profiled(t.tolist(), out[0] if samples else out, max_samples)
        return out

    def conflicts(self, tickets, t_start, pairs=None, t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False, hold_after=False, poses=False):
        """Do the vehicles of the completed, HELD queries `tickets`, each driving its plan on the timetable of the pipeline's last speed_profile call
        from t_start[k] (absolute seconds) on, ever come too close at the same time?  pp_pipeline_conflicts, whose definition is in include/pp_hip.h:
        every plan's pose at the times k * dt inside [t_from, t_to], then for every pair in `pairs` ([n_pairs, 2] indices into `tickets`; None: every
        pair i < j, row-major) the separation of the vehicles' discs (the pipeline's footprint, else the map's min_safe_radius) at the times both are
        present; conflict iff separation < margin.  hold_before / hold_after: a vehicle stands at its first / last sample before its start / behind
        its end instead of being absent.  Nothing but the call's own buffers is written: legal while other queries are in flight.
        Returns (TrajectoryResult per ticket, ConflictResult per pair) and, with poses=True, a list of (T, 3) arrays of (x, y, theta), NaN where the
        vehicle is absent.
        Raises PPError, with nothing launched, for a ticket that is unknown, released, in flight, given twice or without a speed profile (run
        speed_profile first), a t_start that is not finite, a horizon, dt, margin or hold flag outside its domain, fewer than 1 or more than 2^20
        lattice times, a pair index outside the tickets or a pair of a plan with itself."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _conflicts(len(t), t_start, pairs, t_from, t_to, dt, margin, hold_before, hold_after, poses,
                          lambda ts, npairs, pr, cp, xyt, plans, out: self.lib.pp_pipeline_conflicts(self.h, len(t), ptr(t), ptr(ts), npairs, ptr(pr), C.byref(cp), ptr(xyt),
                                                                                                     plans, out))

    def deconflict(self, tickets, t_start, pairs=None, t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False, hold_after=False, max_delay_steps=0):
        """How long must each vehicle of the completed, HELD queries `tickets` wait at its start so that it stays clear of the vehicles above it?
        pp_pipeline_deconflict, whose definition is in include/pp_hip.h.  Priority is the position in `tickets`: of a pair of `pairs` ([n_pairs, 2]
        indices into `tickets`; None: every pair) the larger index yields.  The lattice (t_from, t_to, dt), the margin and the hold flags are those of
        conflicts(); a delay is a whole number of lattice steps, at most max_delay_steps.  In index order every vehicle takes the smallest delay at
        which it is never closer than the margin to a scheduled partner of smaller index; one that finds none gets status 1 and those below it are
        scheduled as if it were absent.  Nothing but the call's own buffers is written: legal while other queries are in flight.
        Returns a numpy record array of DELAY_DTYPE, one record per ticket: status, delay_steps, n_tried, blocker, t_start (the effective start),
        t_block, s_block.
        Raises PPError, with nothing launched, for everything conflicts() refuses (a ticket without a speed profile: run speed_profile first), a
        negative max_delay_steps, or more than 2^20 lattice times and delay steps together."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _deconflict(len(t), t_start, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps,
                           lambda ts, npairs, pr, dp, out: self.lib.pp_pipeline_deconflict(self.h, len(t), ptr(t), ptr(ts), npairs, ptr(pr), C.byref(dp), ptr(out)))

    def deconflict_waits(self, tickets, t_start, pairs=None, no_start_wait=None, fixed=None, t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False,
                         hold_after=False, max_delay_steps=0, max_places=0, places=False):
        """deconflict() for a fleet under way: a vehicle that yields may wait at its start (unless no_start_wait[i]) or at one of the first `max_places`
        stops its timetable reaches inside the horizon -- cusp stops, where it stands anyway.  pp_pipeline_deconflict_waits, whose definition is in
        include/pp_hip.h.  Candidates are tried in the order d = 0, then for d = 1 .. max_delay_steps the start and the places in row order; the first
        clear one is taken.  `fixed` commits waits: None, [n, 2] rows of (row, steps) with row -2 free / -1 the start / >= 0 a stop's row, or the
        record array an earlier call returned (its scheduled vehicles stay bound, wait_fixed()); a fixed vehicle is never decided, only checked
        (status 0, or 2 in conflict; -2 if its row is no stop it reaches in time) and seen by the vehicles below it.
        Returns a numpy record array of WAIT_DTYPE, one record per ticket; with places=True also the listed places [n, max(max_places, 1)]
        (WAIT_PLACE_DTYPE) and their counts [n].
        Raises PPError, with nothing launched, for everything deconflict() refuses, max_places outside 0 .. 2^10, a fixed row below -2 or fixed steps
        outside 0 .. max_delay_steps."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _deconflict_waits(len(t), t_start, no_start_wait, fixed, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps, max_places, places,
                                 lambda ts, flags, fx, npairs, pr, wp, counts, listed, out: self.lib.pp_pipeline_deconflict_waits(
                                     self.h, len(t), ptr(t), ptr(ts), ptr(flags), ptr(fx), npairs, ptr(pr), C.byref(wp), ptr(counts), ptr(listed), ptr(out)))

    def deconflict_tracks(self, tickets, t_start, tracks, pairs=None, t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False, hold_after=False, max_delay_steps=0,
                          details=True):
        """deconflict() with tracked movers: every vehicle of the completed, HELD queries `tickets` gets the smallest start delay at which it is clear of
        the scheduled vehicles above it AND of every track.  pp_pipeline_deconflict_tracks, whose definition is in include/pp_hip.h.  `tracks` is a
        sequence of (radius, waypoints [W, 3]) -- a disc of that radius moving along the rows (t, x, y), t strictly increasing, on straight lines
        between them, absent before its first and behind its last time -- or None for none.  Tracks are never delayed and outrank every vehicle.  With
        max_delay_steps=0 and pairs=[] the call is the plain check of each plan against the movers.  The remaining arguments are deconflict()'s.
        Returns the numpy record array of DELAY_DTYPE -- a blocker >= len(tickets) names track blocker - len(tickets), and s_block[1] is then 0 -- and, with
        details, an [n, M] record array of TRACK_DTYPE: every vehicle against every track at the vehicle's reported candidate (its delay; for status 1
        the largest delay tried).  Without tracks the delay records are deconflict()'s bytes.
        Raises PPError, with nothing launched, for everything deconflict() refuses and for a track set outside its domain (more than 2^16 tracks, 2^24
        waypoints or 2^26 track samples, a value that is not finite, times that do not increase, a negative radius); ValueError for a track whose
        waypoints are not [W, 3] with W >= 1."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _deconflict_tracks(len(t), t_start, tracks, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps, details,
                                  lambda ts, npairs, pr, dp, tk, out, rec: self.lib.pp_pipeline_deconflict_tracks(self.h, len(t), ptr(t), ptr(ts), npairs, ptr(pr), C.byref(dp), tk,
                                                                                                                  ptr(out), ptr(rec)))

    def candidate_pairs(self, tickets, t_start, times_per_box=64, max_delay_steps=0, boxes=False, max_pairs=None, **lattice):
        """Which pairs of the completed, HELD queries `tickets` can meet at all?  The pair list for conflicts(), deconflict() and deconflict_tracks() by a
        space-time broad phase: pp_pipeline_candidate_pairs, whose definition is in include/pp_hip.h.  Per plan and block of `times_per_box` lattice
        times the bounding box of the vehicle's reference point, over every start delay of 0 .. max_delay_steps steps (0 for a list meant for
        conflicts()); a pair is listed when in some block the two boxes are no further apart on either axis than the margin and the footprint allow.
        The list is conservative -- the calls above give the same records over it as over every pair -- ascending in (i, j) and the same bytes on
        every run.  `lattice` are the keywords t_from, t_to, dt, margin, hold_before and hold_after of the call the list is meant for.
        Returns (pairs int32 [P, 2], first_box int32 [P], summary) and, with boxes=True, the [n, NB, 4] boxes (xmin, ymin, xmax, ymax; NaN: the plan
        is absent throughout the block).  summary is a PairSummary: n_found, n_written, n_boxes, reach, n_boxed.  max_pairs=None sizes the buffer and
        calls again once if the list outgrows it; with a number the FIRST max_pairs pairs come back and summary.n_found says how many there are.
        Raises PPError, with nothing launched, for everything deconflict() refuses about tickets, starts, lattice and max_delay_steps, for
        times_per_box outside 1 .. 2^20, max_pairs < 0 and more than 2^26 boxes."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _candidate_pairs(len(t), t_start, times_per_box, max_delay_steps, boxes, max_pairs, lattice,
                                lambda ts, pp, pr, fb, bx, sm: self.lib.pp_pipeline_candidate_pairs(self.h, len(t), ptr(t), ptr(ts), C.byref(pp), ptr(pr), ptr(fb), ptr(bx),
                                                                                                    C.byref(sm)))

    def timetable(self, tickets, values, by="length", max_stops=16):
        """Ask the timetables of the completed, HELD queries `tickets` -- the (s, v, t) rows the last speed_profile() call left on the device -- without
        downloading them: pp_pipeline_timetable, whose definition is in include/pp_hip.h.  `values` is [n, P] (a scalar or [P]: the same for every
        plan): arc lengths in metres with by="length" (the s a locate() call returned gives the set-point speed v, and t, whose difference to the clock
        is the vehicle's lateness and whose now - t is the t_start that re-anchors a vehicle under way for conflicts() and deconflict()), or times in
        seconds since the plan's start with by="time".  Returns three numpy record arrays: plans [n] of TIMETABLE_PLAN_DTYPE (status, n_samples,
        n_stops, n_listed, s_first, s_last, duration), stops [n, max_stops] of TIMETABLE_STOP_DTYPE (row, s, t_arrive, t_depart; the first n_listed
        rows of a plan are its stops in row order -- every sample with v == 0 -- the others zero) and results [n, P] of TIMETABLE_DTYPE (status 0 inside
        the profile, 1 before and 2 behind it, -1 without a profile; row, edge, direction, s, t, v, a, ratio, kappa, pose, next_stop -- an index into the
        plan's listed stops, -1: none -- s_to_stop, t_to_stop, t_remaining).  Legal beside queries in flight.
        Raises PPError, with nothing launched, for everything conflicts() refuses about the tickets and a missing speed profile, for max_stops outside
        0 .. 2^16, more than 2^26 look-ups and a value that is not finite."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _timetable(len(t), values, by, max_stops,
                          lambda P, v, tp, pl, st, out: self.lib.pp_pipeline_timetable(self.h, len(t), ptr(t), P, ptr(v), C.byref(tp), ptr(pl), ptr(st), ptr(out)))

    def retime(self, tickets, holds, rows=False):
        """Write decided waits into the timetables of the completed, HELD queries `tickets` -- the (s, v, t) rows the last speed_profile() call left on the
        device: pp_pipeline_retime, whose definition is in include/pp_hip.h.  `holds` lists (plan, row, seconds), strictly ascending in (plan, row): an
        array of HOLD_DTYPE, [H, 3] numbers, or None / empty for none; plan indexes `tickets`, row is a stop of that plan's profile in 1 .. N - 1, and
        seconds (may be negative) is added to every t_k with k >= row, in place.  wait_holds() turns the records of deconflict_waits() into such a
        list.  Afterwards conflicts(), timetable(), candidate_pairs() and the deconflict calls see the waits; the call accumulates, and a new
        speed_profile() call replaces everything.  A plan is retimed whole or not at all.  Legal beside queries in flight.
        Returns a numpy record array of RETIME_DTYPE, one record per ticket (status 0 applied, -1 no profile, -2 a hold's row is no stop, -3 a hold
        would make a dwell negative; n_holds, first_row, bad_hold, held, duration_before, duration) and, with rows=True, the list of (n_samples, 3)
        arrays of (s, v, t) after the call, as speed_profile() returns them (this object's own speed_profile() call is where their layout is known from).
        Raises PPError, with nothing launched, for everything timetable() refuses about the tickets and a missing speed profile, a plan index outside
        the tickets, a row outside 1 .. N - 1 (a wait at the start is the plan's t_start), seconds that are not finite, a list that is not strictly
        ascending and more than 2^10 holds for one plan."""
        t = np.ascontiguousarray(tickets, dtype=np.uint64).reshape(-1)
        return _retime(len(t), t.tolist(), getattr(self, "_profiled", None), holds, rows,
                       lambda H, hd, buf, out: self.lib.pp_pipeline_retime(self.h, len(t), ptr(t), H, ptr(hd), ptr(buf), ptr(out)))

    def get_expanded_of(self, ticket):
        """expansion sequence (log_expansions=True) of a completed query polled with release=False"""
        slot = self.lib.pp_pipeline_slot_of(self.h, C.c_uint64(int(ticket)))
        if slot < 0:
            raise ValueError("ticket is not a completed, held query")
        n = self._held[int(ticket)].n_expanded
        cells = np.empty((n, 3), dtype=np.int32)
        if n:
            check(self.lib.pp_planner_get_expanded(self.planner_h, slot, ptr(cells)))
        return cells

    def get_obstacle_field_of(self, ticket):
        """the obstacle-heuristic field a completed query polled with release=False was searched with: [rows, cols] float32"""
        slot = self.lib.pp_pipeline_slot_of(self.h, C.c_uint64(int(ticket)))
        if slot < 0:
            raise ValueError("ticket is not a completed, held query")
        out = np.empty((self.map.rows, self.map.cols), dtype=np.float32)
        check(self.lib.pp_planner_get_obstacle_field(self.planner_h, slot, ptr(out)))
        return out

    def close(self):
        if self.h:
            self.lib.pp_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _smoother_params(smoother, params):
    """Smoother::Parameters (smoother.h:28-60, max_curvature = 1 / min_turning_radius) with the fields of the dict `smoother` overridden; None stays NULL:
    the library's defaults, which are the same"""
    if smoother is None:
        return None
    d = dict(step_tolerance=1e-3, max_iterations=2000, learning_rate=0.01, path_weight=0.0, smooth_weight=0.4, voronoi_weight=0.02, collision_weight=0.2,
             curvature_weight=0.4, collision_ratio=0.2, max_curvature=1.0 / params.min_turning_radius)
    d.update(smoother)
    return SmootherParams(**d)


def _processed_path(r, sampled, cusp, smoothed):
    """a processed path as the get_processed_path* calls return it, from its PostResult and arrays; `path` = what HybridAStar::GetPath() returns"""
    return dict(sampled=sampled, cusp=cusp.astype(bool), smoothed=smoothed, status=r.smoothing_status, iterations=r.iterations, length=r.length,
                path=smoothed if r.smoothing_status >= 0 else sampled)


def _per_plan(x, n, dtype=np.float64):
    """a per-plan array of a held-plan call as the C ABI takes it: None stays NULL, a scalar is given to every plan"""
    if x is None:
        return None
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dtype), (n,)) if np.ndim(x) == 0 else x, dtype=dtype).reshape(-1)
    if len(a) != n:
        raise ValueError("one entry per plan: got %d for %d plans" % (len(a), n))
    return a


def _stamp(n, values, from_length, to_length, spacing, margin, call):
    """the per-plan arrays of a stamp call, the call, its records"""
    out = (StampResult * max(n, 1))()
    check(call(_per_plan(values, n, np.int32), _per_plan(from_length, n), _per_plan(to_length, n), StampParams(float(spacing), float(margin), 0), out))
    return list(out)[:n]


SPEED_PROFILE_DEFAULTS = dict(spacing=0.1, v_max_forward=5.0, v_max_reverse=2.0, a_acc=1.5, a_dec=2.5, a_lat=2.0, dwell=0.0, clearance_gain=0.0, v_floor=0.0)


def _speed_profile(n, from_length, to_length, v_start, v_end, max_samples, samples, limits, call):
    """the parameters and per-plan arrays of a speed-profile call, the call, its records and (if wanted) each plan's (s, v, t) rows"""
    unknown = set(limits) - set(SPEED_PROFILE_DEFAULTS)
    if unknown:
        raise TypeError("unknown speed-profile limits: %s" % sorted(unknown))
    sp = SpeedProfileParams(**{k: float(v) for k, v in dict(SPEED_PROFILE_DEFAULTS, **limits).items()})
    out = (SpeedProfileResult * max(n, 1))()
    rows = np.zeros((n, max(int(max_samples), 0), 3)) if samples else None
    check(call(_per_plan(from_length, n), _per_plan(to_length, n), _per_plan(v_start, n), _per_plan(v_end, n), sp, rows, out))
    recs = list(out)[:n]
    if not samples:
        return recs
    return recs, [rows[i, :r.n_samples].copy() if r.status == 0 else np.zeros((0, 3)) for i, r in enumerate(recs)]


def conflict_lattice(t_from, t_to, dt):
    """(k0, T) of the time lattice k * dt inside [t_from, t_to], as the library forms them: tau_m = (k0 + m) * dt for m = 0 .. T - 1"""
    k0, k1 = np.ceil(np.float64(t_from) / np.float64(dt)), np.floor(np.float64(t_to) / np.float64(dt))
    k0, k1 = (int(np.clip(k, -2.0 ** 62, 2.0 ** 62)) if k == k else 2 ** 62 for k in (k0, k1))
    return k0, max(k1 - k0 + 1, 0)


def _conflicts(n, t_start, pairs, t_from, t_to, dt, margin, hold_before, hold_after, poses, call):
    """the parameters, start times and pair list of a conflict call, the call, its plan and pair records and (if wanted) each plan's (x, y, theta) per lattice time"""
    cp = ConflictParams(float(t_from), float(t_to), float(dt), float(margin), int(hold_before), int(hold_after))
    ts = _per_plan(t_start, n)
    if ts is None and n:
        raise ValueError("one start time per plan")
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n_pairs = n * (n - 1) // 2 if pr is None else len(pr)
    xyt = None
    if poses:
        T = conflict_lattice(t_from, t_to, dt)[1] if float(dt) > 0.0 and np.isfinite([t_from, t_to, dt]).all() else 0
        xyt = np.full((n, T if T <= 1 << 20 else 0, 3), np.nan)
    plans, out = (TrajectoryResult * max(n, 1))(), (ConflictResult * max(n_pairs, 1))()
    check(call(ts, n_pairs, pr, cp, xyt, plans, out))
    recs = (list(plans)[:n], list(out)[:n_pairs])
    return recs + ([xyt[i] for i in range(n)],) if poses else recs


# pp_delay_result as a numpy record: a deconflict call returns one array of these, not one object per record
DELAY_DTYPE = np.dtype([("status", np.int32), ("delay_steps", np.int32), ("n_tried", np.int32), ("blocker", np.int32), ("t_start", np.float64), ("t_block", np.float64),
                        ("s_block", np.float64, (2,))])
assert DELAY_DTYPE.itemsize == C.sizeof(DelayResult)


def delay_levels(n, pairs):
    """the level each of n vehicles is decided on by a deconflict call with the pair list `pairs` ([n_pairs, 2]; None: every pair): 0 without a pair
    partner of smaller index, else one more than the highest level among those partners.  The call makes one kernel launch per level."""
    if pairs is None:
        return np.arange(n, dtype=np.int32)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    below = [[] for _ in range(n)]
    for lo, hi in zip(pr.min(axis=1).tolist(), pr.max(axis=1).tolist()):
        below[hi].append(lo)
    level = np.zeros(n, dtype=np.int32)
    for i in range(n):
        level[i] = max((level[j] + 1 for j in below[i]), default=0)
    return level


def _deconflict(n, t_start, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps, call):
    """the parameters, start times and pair list of a delay call, the call, its records as one numpy record array"""
    dp = DelayParams(ConflictParams(float(t_from), float(t_to), float(dt), float(margin), int(hold_before), int(hold_after)), int(max_delay_steps), 0)
    ts = _per_plan(t_start, n)
    if ts is None and n:
        raise ValueError("one start time per plan")
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n_pairs = n * (n - 1) // 2 if pr is None else len(pr)
    out = np.zeros(max(n, 1), dtype=DELAY_DTYPE)
    check(call(ts, n_pairs, pr, dp, out))
    return out[:n].view(np.recarray)


# pp_wait_result, pp_wait_place and pp_wait_fixed as numpy records
WAIT_DTYPE = np.dtype([("status", np.int32), ("place", np.int32), ("row", np.int32), ("wait_steps", np.int32), ("n_tried", np.int32), ("blocker", np.int32),
                       ("t_start", np.float64), ("t_hold", np.float64), ("t_resume", np.float64), ("s_wait", np.float64), ("t_block", np.float64), ("s_block", np.float64, (2,))])
WAIT_PLACE_DTYPE = np.dtype([("row", np.int32), ("column", np.int32), ("s", np.float64), ("t_arrive", np.float64), ("pose", np.float64, (3,)), ("sin_theta", np.float64),
                             ("cos_theta", np.float64)])
WAIT_FIXED_DTYPE = np.dtype([("row", np.int32), ("steps", np.int32)])
assert WAIT_DTYPE.itemsize == C.sizeof(WaitResult) and WAIT_PLACE_DTYPE.itemsize == C.sizeof(WaitPlace) and WAIT_FIXED_DTYPE.itemsize == C.sizeof(WaitFixed)


def wait_fixed(fixed, n):
    """the committed waits of a deconflict_waits call as an array of WAIT_FIXED_DTYPE: None; an array of that dtype; [n, 2] integers (row, steps); or
    the record array of an earlier call, whose scheduled vehicles (status 0 or 2) stay bound by what they were given -- a wait at the start (also one
    of no steps) as row -1, a wait at a stop as its row -- and whose other vehicles are free (row -2)"""
    if fixed is None:
        return None
    if isinstance(fixed, np.ndarray) and fixed.dtype.names and "wait_steps" in fixed.dtype.names:
        if len(fixed) != n:
            raise ValueError("one committed wait per plan")
        out = np.zeros(n, dtype=WAIT_FIXED_DTYPE)
        bound = (fixed["status"] == 0) | (fixed["status"] == 2)
        out["row"] = np.where(bound, np.where(fixed["place"] >= 0, fixed["row"], -1), -2)
        out["steps"] = np.where(bound, fixed["wait_steps"], 0)
        return out
    if isinstance(fixed, np.ndarray) and fixed.dtype == WAIT_FIXED_DTYPE:
        out = np.ascontiguousarray(fixed).reshape(-1)
    else:
        pairs = np.asarray(fixed, dtype=np.int64).reshape(-1, 2)
        if len(pairs) and (np.abs(pairs) >= 2 ** 31).any():
            raise ValueError("a committed wait is (row, steps) in int32")
        out = np.zeros(len(pairs), dtype=WAIT_FIXED_DTYPE)
        out["row"], out["steps"] = pairs[:, 0], pairs[:, 1]
    if len(out) != n:
        raise ValueError("one committed wait per plan")
    return out


def _deconflict_waits(n, t_start, no_start_wait, fixed, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps, max_places, places, call):
    """the parameters, start times, flags, committed waits and pair list of a call with waits at stops, the call, its records as one numpy record array
    and (places=True) the listed places [n, max(max_places, 1)] and their counts [n]"""
    wp = WaitParams(DelayParams(ConflictParams(float(t_from), float(t_to), float(dt), float(margin), int(hold_before), int(hold_after)), int(max_delay_steps), 0),
                    int(max_places), 0)
    ts = _per_plan(t_start, n)
    if ts is None and n:
        raise ValueError("one start time per plan")
    flags = None
    if no_start_wait is not None:
        flags = np.asarray(no_start_wait)
        flags = np.full(n, bool(flags), dtype=np.uint8) if flags.ndim == 0 else np.ascontiguousarray(flags.reshape(-1) != 0, dtype=np.uint8)
        if len(flags) != n:
            raise ValueError("one no_start_wait flag per plan")
    fx = wait_fixed(fixed, n)
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n_pairs = n * (n - 1) // 2 if pr is None else len(pr)
    out = np.zeros(max(n, 1), dtype=WAIT_DTYPE)
    stride = max(int(max_places), 1) if 0 <= int(max_places) <= 1 << 10 else 1
    listed = np.zeros((max(n, 1), stride), dtype=WAIT_PLACE_DTYPE) if places else None
    counts = np.zeros(max(n, 1), dtype=np.int32) if places else None
    check(call(ts, flags, fx, n_pairs, pr, wp, counts, listed, out))
    recs = out[:n].view(np.recarray)
    return (recs, listed[:n].view(np.recarray), counts[:n]) if places else recs


def _box_count(t_from, t_to, dt, times_per_box):
    """NB of a candidate_pairs call, to size its boxes: ceil(T / B) with T the lattice times k * dt of [t_from, t_to]; 1 for arguments the call refuses"""
    with np.errstate(all="ignore"):
        T = conflict_lattice(t_from, t_to, dt)[1]
    B = int(times_per_box)
    return -(-T // B) if 1 <= T <= 1 << 20 and B >= 1 else 1


def _candidate_pairs(n, t_start, times_per_box, max_delay_steps, boxes, max_pairs, lattice, call):
    """the parameters and start times of a broad-phase call, the call (twice if the list outgrows a buffer sized here), the list, the first box of every
    pair, the summary and (if wanted) the boxes"""
    unknown = set(lattice) - {"t_from", "t_to", "dt", "margin", "hold_before", "hold_after"}
    if unknown:
        raise TypeError("candidate_pairs: unexpected keyword %s" % ", ".join(sorted(unknown)))
    kw = dict(dict(t_from=0.0, t_to=60.0, dt=0.1, margin=0.0, hold_before=False, hold_after=False), **lattice)
    cp = ConflictParams(float(kw["t_from"]), float(kw["t_to"]), float(kw["dt"]), float(kw["margin"]), int(kw["hold_before"]), int(kw["hold_after"]))
    ts = _per_plan(t_start, n)
    if ts is None and n:
        raise ValueError("one start time per plan")
    every = n * (n - 1) // 2
    room = min(every, max(1024, 8 * n)) if max_pairs is None else int(max_pairs)
    box = np.zeros((n, _box_count(kw["t_from"], kw["t_to"], kw["dt"], times_per_box), 4)) if boxes else None
    while True:
        pp = PairParams(DelayParams(cp, int(max_delay_steps), 0), int(times_per_box), room)
        pairs, first, summary = np.zeros((max(room, 1), 2), dtype=np.int32), np.zeros(max(room, 1), dtype=np.int32), PairSummary()
        check(call(ts, pp, pairs if room > 0 else None, first if room > 0 else None, box if box is not None and box.size else None, summary))
        if max_pairs is not None or summary.n_found <= room:
            break
        room = int(summary.n_found)
    if box is not None and n:
        assert box.shape[1] == summary.n_boxes, (box.shape, summary.n_boxes)
    out = (pairs[:summary.n_written], first[:summary.n_written], summary)
    return out + (box,) if boxes else out


# pp_timetable_plan, pp_timetable_stop and pp_timetable_result as numpy records: what a timetable call returns
TIMETABLE_PLAN_DTYPE = np.dtype([("status", np.int32), ("n_samples", np.int32), ("n_stops", np.int32), ("n_listed", np.int32), ("s_first", np.float64), ("s_last", np.float64),
                                 ("duration", np.float64)])
TIMETABLE_STOP_DTYPE = np.dtype([("row", np.int32), ("reserved", np.int32), ("s", np.float64), ("t_arrive", np.float64), ("t_depart", np.float64)])
TIMETABLE_DTYPE = np.dtype([("status", np.int32), ("row", np.int32), ("edge", np.int32), ("direction", np.int32), ("s", np.float64), ("t", np.float64), ("v", np.float64),
                            ("a", np.float64), ("ratio", np.float64), ("kappa", np.float64), ("pose", np.float64, 3), ("next_stop", np.int32), ("reserved", np.int32),
                            ("s_to_stop", np.float64), ("t_to_stop", np.float64), ("t_remaining", np.float64), ("reserved1", np.float64)])
assert TIMETABLE_PLAN_DTYPE.itemsize == C.sizeof(TimetablePlan) and TIMETABLE_STOP_DTYPE.itemsize == C.sizeof(TimetableStop) and TIMETABLE_DTYPE.itemsize == C.sizeof(TimetableResult)


def _timetable(n, values, by, max_stops, call):
    """the values and parameters of a timetable call, the call, its three record arrays (no object per record)"""
    if by not in ("length", "time"):
        raise ValueError('by is "length" or "time", got %r' % (by,))
    v = np.asarray(values, dtype=np.float64)
    if v.ndim < 2:
        v = np.broadcast_to(v.reshape(1, -1), (n, v.size))
    if v.ndim != 2 or v.shape[0] != n:
        raise ValueError("values is [n, P] with one row per plan: got %s for %d plans" % (v.shape, n))
    v = np.ascontiguousarray(v)
    P, M = int(v.shape[1]), int(max_stops)
    plans = np.zeros(max(n, 1), dtype=TIMETABLE_PLAN_DTYPE)
    stops = np.zeros((max(n, 1), max(M, 1)), dtype=TIMETABLE_STOP_DTYPE)
    out = np.zeros((max(n, 1), max(P, 1)), dtype=TIMETABLE_DTYPE)
    check(call(P, v if v.size else None, TimetableParams(0 if by == "length" else 1, M), plans, stops, out))
    return plans[:n].view(np.recarray), stops[:n, :max(M, 0)].view(np.recarray), out[:n, :P].view(np.recarray)


# pp_hold and pp_retime_result as numpy records: what a retime call takes and returns
HOLD_DTYPE = np.dtype([("plan", np.int32), ("row", np.int32), ("seconds", np.float64)])
RETIME_DTYPE = np.dtype([("status", np.int32), ("n_holds", np.int32), ("first_row", np.int32), ("bad_hold", np.int32), ("held", np.float64), ("duration_before", np.float64),
                         ("duration", np.float64)])
assert HOLD_DTYPE.itemsize == C.sizeof(Hold) and RETIME_DTYPE.itemsize == C.sizeof(RetimeResult)


def _profiled(keys, recs, max_samples):
    """what a wrapper object remembers of its last speed_profile call for retime(rows=True): the stride of the rows and every plan's sample count"""
    return int(max_samples), {int(k): (int(r.n_samples) if r.status == 0 else 0) for k, r in zip(keys, recs)}


def hold_list(holds):
    """the holds of a retime call as an array of HOLD_DTYPE: None or empty; an array of that dtype; or [H, 3] numbers (plan, row, seconds)"""
    if holds is None:
        return np.zeros(0, dtype=HOLD_DTYPE)
    if isinstance(holds, np.ndarray) and holds.dtype == HOLD_DTYPE:
        return np.ascontiguousarray(holds).reshape(-1)
    rows = np.asarray(holds, dtype=np.float64).reshape(-1, 3)
    if len(rows) and not (np.isfinite(rows[:, :2]).all() and (rows[:, :2] == np.rint(rows[:, :2])).all() and (np.abs(rows[:, :2]) < 2 ** 31).all()):
        raise ValueError("a hold is (plan, row, seconds) with plan and row in int32")
    out = np.zeros(len(rows), dtype=HOLD_DTYPE)
    out["plan"], out["row"], out["seconds"] = rows[:, 0], rows[:, 1], rows[:, 2]
    return out


def _retime(n, keys, profiled, holds, rows, call):
    """the hold list of a retime call, the call, its records as one numpy record array and (rows=True) each plan's (s, v, t) rows after it"""
    hd = hold_list(holds)
    if rows and n and profiled is None:
        raise ValueError("rows=True needs the layout of the rows: call this object's speed_profile() first")
    buf = np.zeros((n, profiled[0] if profiled else 0, 3)) if rows else None
    out = np.zeros(max(n, 1), dtype=RETIME_DTYPE)
    check(call(len(hd), hd if len(hd) else None, buf if rows and buf.size else None, out))
    recs = out[:n].view(np.recarray)
    if not rows:
        return recs
    return recs, [buf[i, :profiled[1].get(int(k), 0)].copy() if recs[i].status != -1 else np.zeros((0, 3)) for i, k in enumerate(keys)]


def wait_holds(results, dt, t_start):
    """The record array of a deconflict_waits() call as what commits it: (holds, t_start').  A scheduled vehicle (status 0 or 2) that waits
    wait_steps > 0 steps at a stop (place >= 0) becomes the hold (i, row, wait_steps * dt) for retime(); one that waits at its start gets the
    record's effective t_start; every other vehicle keeps its t_start.  After retime(tickets, holds) the calls that take start times see the
    schedule the call decided under t_start', and a next deconflict_waits() round needs no `fixed` entry for these vehicles."""
    n = len(results)
    ts = np.array(_per_plan(t_start, n), dtype=np.float64).reshape(-1)
    bound = (results["status"] == 0) | (results["status"] == 2)
    at_stop = bound & (results["place"] >= 0) & (results["wait_steps"] > 0)
    at_start = bound & (results["place"] == -1)
    ts[at_start] = results["t_start"][at_start]
    k = np.flatnonzero(at_stop)
    holds = np.zeros(len(k), dtype=HOLD_DTYPE)
    holds["plan"], holds["row"], holds["seconds"] = k, results["row"][k], results["wait_steps"][k].astype(np.float64) * np.float64(dt)
    return holds, ts


# pp_track_result as a numpy record: a deconflict_tracks call returns an [n, M] array of these
TRACK_DTYPE = np.dtype([("status", np.int32), ("n_times", np.int32), ("n_conflict", np.int32), ("reserved", np.int32), ("t_first", np.float64), ("s_first", np.float64),
                        ("min_separation", np.float64), ("t_min", np.float64), ("s_min", np.float64), ("reserved1", np.float64)])
assert TRACK_DTYPE.itemsize == C.sizeof(TrackResult)


def track_set(tracks):
    """(TrackSet, the arrays it points into) of a sequence of (radius, waypoints [W, 3]); None: no track.  The arrays must outlive the call."""
    tracks = [] if tracks is None else list(tracks)
    offsets, rows, radii = [0], [], []
    for k, (radius, waypoints) in enumerate(tracks):
        w = np.asarray(waypoints, dtype=np.float64)
        if w.ndim != 2 or w.shape[1] != 3 or len(w) < 1:
            raise ValueError("track %d: waypoints are [W, 3] rows (t, x, y) with W >= 1, got shape %s" % (k, w.shape))
        rows.append(w)
        offsets.append(offsets[-1] + len(w))
        radii.append(float(radius))
    keep = (np.array(offsets, dtype=np.int32), np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 3))), np.array(radii, dtype=np.float64))
    return TrackSet(len(tracks), 0, *(a.ctypes.data for a in keep)), keep


def _deconflict_tracks(n, t_start, tracks, pairs, t_from, t_to, dt, margin, hold_before, hold_after, max_delay_steps, details, call):
    """the parameters, start times, pair list and track set of a delay call with tracked movers, the call, its records as numpy record arrays"""
    dp = DelayParams(ConflictParams(float(t_from), float(t_to), float(dt), float(margin), int(hold_before), int(hold_after)), int(max_delay_steps), 0)
    ts = _per_plan(t_start, n)
    if ts is None and n:
        raise ValueError("one start time per plan")
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n_pairs = n * (n - 1) // 2 if pr is None else len(pr)
    tk, keep = (None, None) if tracks is None else track_set(tracks)
    M = 0 if tk is None else tk.n_tracks
    out = np.zeros(max(n, 1), dtype=DELAY_DTYPE)
    rec = np.zeros((n, M), dtype=TRACK_DTYPE) if details else None
    check(call(ts, n_pairs, pr, dp, None if tk is None else C.byref(tk), out, rec if rec is not None and rec.size else None))
    del keep
    out = out[:n].view(np.recarray)
    return (out, rec.view(np.recarray)) if details else out


def _locate(n, poses, from_length, to_length, spacing, heading_weight, call):
    """the vehicle poses and per-plan arrays of a locate call, the call, its records"""
    v = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    if len(v) != n:
        raise ValueError("one vehicle pose per plan: got %d for %d plans" % (len(v), n))
    out = (LocateResult * max(n, 1))()
    check(call(v, _per_plan(from_length, n), _per_plan(to_length, n), LocateParams(float(spacing), float(heading_weight)), out))
    return list(out)[:n]


class _RRTBase:
    """RRT / RRTStar over R2 (algo/rrt.h, algo/rrt_star.h): the whole sequential loop runs on the device.
    validator=None reproduces StateValidatorFree (planner/tests/test_rrt*.cpp)."""
    _star = 0

    def __init__(self, ctx, lower, upper, validator=None, max_iteration=None, max_number_tree_node=10000, max_connection_distance=0.1,
                 goal_bias=0.05, rewire=False, radius_gamma=None):
        """rewire / radius_gamma (RRTStar only) go beyond the reference, whose RRT* has no rewire step (rrt_star.h:83): rewire=True
        re-parents near nodes through the new node and carries the saving down their subtrees; radius_gamma=g also replaces the
        k-nearest near-set by the <= 16 nearest nodes within g * sqrt(ln(n + 1) / (n + 1))."""
        self.ctx = ctx
        self.lib = ctx.lib
        if self._star and (rewire or radius_gamma is not None):
            self._star = 3 if radius_gamma is not None else 2
        self.gamma = float(radius_gamma) if radius_gamma is not None else 0.0
        self.lower = np.ascontiguousarray(lower, dtype=np.float64)[:2].copy()
        self.upper = np.ascontiguousarray(upper, dtype=np.float64)[:2].copy()
        self.validator = validator
        if max_iteration is None:
            max_iteration = 10000 if self._star else 100  # RRTStarParameters / RRTParameters defaults
        self.max_iteration = max_iteration
        self.max_number_tree_node = max_number_tree_node
        self.max_connection_distance = max_connection_distance
        self.goal_bias = goal_bias
        self._init = np.zeros(2)
        self._goal = np.zeros(2)
        self._seed = 0
        self.result = None

    def set_init_state(self, p):
        self._init = np.ascontiguousarray(p, dtype=np.float64)[:2].copy()

    def set_goal_state(self, p):
        self._goal = np.ascontiguousarray(p, dtype=np.float64)[:2].copy()

    def set_seed(self, seed):
        self._seed = int(seed)

    def search_path(self):
        params = np.array([self.max_iteration, self.max_number_tree_node, self.max_connection_distance, self.goal_bias, self.gamma], dtype=np.float64)
        h = C.c_void_p()
        res = _lib.RrtResult()
        mh = self.validator.map.h if self.validator is not None else None
        check(self.lib.pp_rrt_run(self.ctx.h, mh, ptr(self.lower), ptr(self.upper), ptr(params), ptr(self._init), ptr(self._goal),
                                  C.c_uint64(self._seed), self._star, C.byref(h), C.byref(res)))
        nodes = np.empty((res.n_nodes, 2))
        parents = np.empty(res.n_nodes, dtype=np.int32)
        costs = np.empty(res.n_nodes)
        path = np.empty((res.n_path, 2))
        check(self.lib.pp_rrt_get(h, ptr(nodes), ptr(parents), ptr(costs), ptr(path)))
        self.lib.pp_rrt_destroy(h)
        self.result = dict(status=res.status, nodes=nodes, parents=parents, costs=costs, path=path, iterations=res.iterations,
                           n_knn=res.n_knn_queries, n_edge_checks=res.n_edge_checks)
        return Status.SUCCESS if res.status == 0 else Status.FAILURE

    def get_path(self):
        return self.result["path"] if self.result is not None else np.empty((0, 2))

    def search_batch(self, inits, goals, seeds):
        """n independent problems (own start, goal, seed), one workgroup each, run together on the GPU.
        Returns one result dict per problem (same fields as `self.result`)."""
        inits = np.ascontiguousarray(inits, dtype=np.float64).reshape(-1, 2)
        goals = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        n = len(inits)
        assert goals.shape == inits.shape and seeds.shape == (n,)
        params = np.array([self.max_iteration, self.max_number_tree_node, self.max_connection_distance, self.goal_bias, self.gamma], dtype=np.float64)
        hs = (C.c_void_p * n)()
        res = (_lib.RrtResult * n)()
        mh = self.validator.map.h if self.validator is not None else None
        check(self.lib.pp_rrt_run_batch(self.ctx.h, mh, ptr(self.lower), ptr(self.upper), ptr(params), n, ptr(inits), ptr(goals), ptr(seeds), self._star,
                                        C.cast(hs, C.POINTER(C.c_void_p)), res))
        out = []
        for i in range(n):
            nodes = np.empty((res[i].n_nodes, 2))
            parents = np.empty(res[i].n_nodes, dtype=np.int32)
            costs = np.empty(res[i].n_nodes)
            path = np.empty((res[i].n_path, 2))
            h = C.c_void_p(hs[i])
            check(self.lib.pp_rrt_get(h, ptr(nodes), ptr(parents), ptr(costs), ptr(path)))
            self.lib.pp_rrt_destroy(h)
            out.append(dict(status=res[i].status, nodes=nodes, parents=parents, costs=costs, path=path, iterations=res[i].iterations,
                            n_knn=res[i].n_knn_queries, n_edge_checks=res[i].n_edge_checks))
        return out


class RRT(_RRTBase):
    _star = 0


class RRTStar(_RRTBase):
    _star = 1


class GridAStarBatch:
    """AStarN2 / BidirectionalAStarN2 (algo/a_star_n2.h, algo/bidirectional_a_star.h) for many (init, goal) pairs at once, one wave per
    query on the device, with the transition cost and heuristic of the reference's script (example_a_star_grid.py:46-52: Euclidean
    distance between cells).  Other cost / heuristic functions run on the host engine (pyplanning.AStarN2, per-edge callbacks as in
    the reference)."""

    def __init__(self, map_set):
        self.map = map_set
        self.lib = map_set.lib

    def search_batch(self, inits, goals, bidirectional=False, inner_goals=None, max_path=None, max_expanded=None, want_expanded=None):
        """inits / goals: [n][2] (row, col).  inner_goals [n][4] (bidirectional only): the goals held by the two heuristics the
        AverageHeuristic pair wraps (default: forward -> goal, reverse -> init).  Returns one dict per query: status, cost, path
        [(row, col)], n_expanded and -- want_expanded (default: while n * cells <= 2^26) -- expanded (expansion order; + expanded_reverse
        when bidirectional)."""
        inits = np.ascontiguousarray(inits, dtype=np.int32).reshape(-1, 2)
        goals = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
        n = len(inits)
        assert goals.shape == inits.shape
        cells = self.map.rows * self.map.cols
        if want_expanded is None:  # the expansion orders are [n][cells][2] int32 per direction: only while that stays small
            want_expanded = max_expanded is not None or n * cells <= (1 << 26)
        max_path = int(max_path) if max_path is not None else min(cells + 1, 4 * (self.map.rows + self.map.cols))
        max_expanded = int(max_expanded) if max_expanded is not None else (cells if want_expanded else 0)
        ig = None
        if inner_goals is not None:
            ig = np.ascontiguousarray(inner_goals, dtype=np.int32).reshape(n, 4)
        res = (_lib.GridResult * max(n, 1))()
        paths = np.zeros((n, max_path, 2), dtype=np.int32)
        exp = np.zeros((n, max_expanded, 2), dtype=np.int32) if want_expanded else None
        expr = np.zeros((n, max_expanded, 2), dtype=np.int32) if want_expanded and bidirectional else None
        check(self.lib.pp_grid_astar_batch(self.map.h, n, ptr(inits), ptr(goals), 1 if bidirectional else 0, ptr(ig) if ig is not None else None,
                                           max_path, max_expanded if want_expanded else 0, res, ptr(paths), ptr(exp) if exp is not None else None,
                                           ptr(expr) if expr is not None else None))
        out = []
        for i in range(n):
            r = res[i]
            if r.n_path > max_path or (want_expanded and max(r.n_expanded, r.n_expanded_reverse) > max_expanded):
                raise _lib.PPError("query %d: path (%d) or expansion list (%d) longer than the buffers" % (i, r.n_path, r.n_expanded))
            d = dict(status=r.status, cost=r.cost, path=paths[i, :r.n_path].copy(), n_expanded=r.n_expanded, n_expanded_reverse=r.n_expanded_reverse)
            if want_expanded:
                d["expanded"] = exp[i, :r.n_expanded].copy()
                if bidirectional:
                    d["expanded_reverse"] = expr[i, :r.n_expanded_reverse].copy()
            out.append(d)
        return out
