"""-m gpu: the obstacle heuristic with a clearance radius (include/pp_hip.h, "heuristic clearance"): for the heuristic only, a cell is
blocked iff it is occupied or !(dist >= radius).

The oracle side of every comparison is the unchanged CPU oracle on an INFLATED occupancy grid: a World is built, its d2 and occ are read,
occ2 = where(float32(sqrt(d2) * res) >= float32(radius), occ, 0) keeps the original obstacle ids, and set_occ(occ2) / set_d2(d2) install
the pair.  Fields come from World.obstacle_heuristic, searches from Hybrid.search with one table for both sides.  Oracle fields and
searches are computed once per module and shared by the tests that need them."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import footprint_ref as R
import oracle_lib as O
from gpu_common import make_pair, rect_vertices, valid_random_poses
from test_gpu_hybrid import compare
from test_gpu_pipeline import check_against_oracle
from test_gpu_pipeline_footprint import assert_is_the_one_wave_search, run_pipe, yardstick

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.1
RADII = (0.35, 1.0)  # below two cells at 0.1 m; the validator's default minSafeRadius
PP_ERR_INVALID = -1

# (rows, cols, outlines, seed): a multiple of the tile, and three ragged grids -- the last bit word of a row and the tile halo
FIELD_GRIDS = ((96, 96, 3, 3), (200, 333, 8, 5), (129, 127, 4, 7), (65, 64, 2, 9))


# ------------------------------------------------------------------------------------------------------ oracle --
def blocked_mask(d2, occ, radius, resolution=RES):
    """the definition: occupied, or !(dist >= radius) with the map's float distance (gvd.h:38: double sqrt times the float resolution, as float)"""
    dist = (np.sqrt(d2.astype(np.float64)) * np.float64(np.float32(resolution))).astype(np.float32)
    return (occ >= 0) | ~(dist >= np.float32(radius))


def inflate(w, radius, occ=None, d2=None):
    """installs the inflated occupancy in the oracle world `w` (its own grids unless given); the original occupied ids are kept"""
    d2 = w.d2().copy() if d2 is None else d2
    occ = w.occ().copy() if occ is None else occ
    dist = (np.sqrt(d2.astype(np.float64)) * np.float64(np.float32(RES))).astype(np.float32)
    occ2 = np.where(dist >= np.float32(radius), -1, 0).astype(np.int32)
    occ2[occ >= 0] = occ[occ >= 0]
    assert np.array_equal(occ2 >= 0, blocked_mask(d2, occ, radius))
    w.set_occ(occ2)
    w.set_d2(d2)
    return w


def grid_world(rows, cols, n_obstacles, seed):
    hx, hy = rows * RES / 2, cols * RES / 2
    w = O.synthetic_world(0, n_obstacles, seed, RES, lower=(-hx, -hy), upper=(hx, hy))
    assert (w.rows, w.cols) == (rows, cols)
    return w


def cell_centre(w, r, c):
    return (w.origin[0] + (r + 0.5) * RES, w.origin[1] + (c + 0.5) * RES)


@functools.lru_cache(maxsize=None)
def field_goals(grid, radius):
    """40 goals: the four corners, a FREE cell with dist < radius (blocked for the heuristic, still costs 0 as the goal), an occupied cell,
    a goal outside the map, and 33 random ones"""
    rows, cols, n_obstacles, seed = grid
    w = grid_world(*grid)
    hx, hy = rows * RES / 2, cols * RES / 2
    occ, d2 = w.occ(), w.d2()
    goals = [(-hx + 0.01, -hy + 0.01), (hx - 0.01, hy - 0.01), (hx - 0.01, -hy + 0.01), (-hx + 0.01, hy - 0.01)]
    near = np.argwhere(blocked_mask(d2, occ, radius) & (occ < 0))
    assert len(near), "no free cell closer than the radius"
    goals.append(cell_centre(w, *near[len(near) // 2]))
    occupied = np.argwhere(occ >= 0)
    assert len(occupied)
    goals.append(cell_centre(w, *occupied[len(occupied) // 2]))
    goals.append((hx + 5.0, 0.0))
    rng = np.random.RandomState(seed * 100 + int(radius * 100))
    goals += [tuple(x) for x in rng.uniform([-hx, -hy], [hx, hy], (33, 2))]
    assert len(goals) == 40
    return tuple(goals)


@functools.lru_cache(maxsize=None)
def oracle_fields(grid, radius):
    w = inflate(grid_world(*grid), radius)
    out = np.stack([w.obstacle_heuristic(g)[0] for g in field_goals(grid, radius)])
    out.setflags(write=False)
    return out


def device_grid(grid, ctx=None, path_cost=False):
    import pathplanning_amd as pa
    w = grid_world(*grid)
    ctx = ctx or pa.Context(0)
    ms = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, RES)
    assert (ms.rows, ms.cols) == (w.rows, w.cols)
    ms.upload_dist2(w.d2())
    ms.upload_occupancy(w.occ())
    if path_cost:
        ms.upload_path_cost(w.pathcost())
    return w, ms, ctx


def device_fields():
    """{(grid index, radius): [40, rows, cols]} through the public stand-alone entry, whatever form of the wavefront the environment selects"""
    import pathplanning_amd as pa
    out, ctx = {}, None
    for gi, grid in enumerate(FIELD_GRIDS):
        w, ms, ctx = device_grid(grid, ctx)
        for radius in RADII:
            out[(gi, radius)] = pa.ObstaclesHeuristic(ms).update(field_goals(grid, radius), clearance=radius)
    return out


def assert_fields(got):
    for gi, grid in enumerate(FIELD_GRIDS):
        for radius in RADII:
            want = oracle_fields(grid, radius)
            g = got[(gi, radius)]
            assert g.shape == want.shape
            for i in range(len(want)):
                assert np.array_equal(g[i].view(np.uint32), want[i].view(np.uint32)), (grid, radius, i, field_goals(grid, radius)[i])


# ------------------------------------------------------------------------------------------------ 1: the fields --
def test_special_goals_are_what_they_claim():
    """the yardstick's own cases: the near-obstacle goal is free, blocked by the radius, and costs 0 in a field that is not empty; the
    outside goal's field is +inf everywhere; with the clearance some cells that the plain rule reaches are +inf"""
    for grid in FIELD_GRIDS:
        w = grid_world(*grid)
        occ, d2 = w.occ(), w.d2()
        for radius in RADII:
            goals, want = field_goals(grid, radius), oracle_fields(grid, radius)
            r, c = w.to_cell([goals[4]])[0]
            assert occ[r, c] < 0 and blocked_mask(d2, occ, radius)[r, c] and want[4][r, c] == 0.0
            r, c = w.to_cell([goals[5]])[0]
            assert occ[r, c] >= 0 and want[5][r, c] == 0.0
            assert np.isinf(want[6]).all()
            for i in (0, 7, 20):  # a corner and two random goals: blocked cells keep +inf (the goal's own cell costs 0), and the plain rule reaches more
                plain = w.obstacle_heuristic(goals[i])[0]
                others = blocked_mask(d2, occ, radius)
                r, c = w.to_cell([goals[i]])[0]
                others[r, c] = False
                assert want[i][r, c] == 0.0 and np.isinf(want[i][others]).all()
                assert (np.isfinite(plain) & np.isinf(want[i])).any()


def test_fields_equal_the_oracle():
    assert_fields(device_fields())


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_heuristic_clearance as T
got = T.device_fields()
np.savez(sys.argv[2], **{"%d_%s" % k: v for k, v in got.items()})
print("DONE", len(got))
"""


def _fields_from_child(tmp_path, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    out = str(tmp_path / "fields.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE 8" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
    z = np.load(out)
    return {(gi, radius): z["%d_%s" % (gi, radius)] for gi in range(len(FIELD_GRIDS)) for radius in RADII}


def test_fields_through_the_ordered_kernel(tmp_path):
    """PP_WF_TILES=0: every goal through the ordered kernel, which reads the blocked BYTE grid"""
    assert_fields(_fields_from_child(tmp_path, {"PP_WF_TILES": "0"}))


def test_fields_with_forced_hand_over(tmp_path):
    """PP_WF_TILES_FORCE_FALLBACK=3: every third goal is handed by the tile form (bit rows) to the ordered kernel (bytes) in one launch"""
    assert_fields(_fields_from_child(tmp_path, {"PP_WF_TILES_FORCE_FALLBACK": "3"}))


# ------------------------------------------------------------------------------------------- 2: radius 0 is off --
def test_radius_zero_is_todays_entry_bit_for_bit():
    import pathplanning_amd as pa
    from pathplanning_amd._lib import ptr
    grid = FIELD_GRIDS[1]
    w, ms, ctx = device_grid(grid)
    goals = np.ascontiguousarray(field_goals(grid, 1.0), dtype=np.float64)
    want = pa.ObstaclesHeuristic(ms).update(goals)
    got = np.full_like(want, -1.0)
    assert ms.lib.pp_obstacle_heuristic_clearance(ms.h, C.c_float(0.0), len(goals), ptr(goals), ptr(got)) == 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(pa.ObstaclesHeuristic(ms).update(goals, clearance=1.0).view(np.uint32), want.view(np.uint32))
    # a map that has no distance grid: radius 0 still is the plain entry
    ms2 = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, RES)
    ms2.upload_occupancy(w.occ())
    got2 = np.full_like(want, -1.0)
    assert ms2.lib.pp_obstacle_heuristic_clearance(ms2.h, C.c_float(0.0), len(goals), ptr(goals), ptr(got2)) == 0
    assert np.array_equal(got2.view(np.uint32), want.view(np.uint32))


def test_a_planner_set_to_zero_is_a_planner_never_set():
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    rng = np.random.RandomState(31)
    n = 12
    starts, goals = valid_random_poses(rng, w, n), valid_random_poses(rng, w, n)
    seeds = np.arange(n, dtype=np.uint64) + 50
    plain = pa.HybridAStarBatch(val, max_batch=n, max_nodes=32768)
    plain.initialize()
    assert plain.heuristic_clearance == 0.0
    want = yardstick(plain, starts, goals, seeds)
    zero = pa.HybridAStarBatch(val, max_batch=n, max_nodes=32768)
    zero.initialize(plain.nonholo_table())
    zero.set_heuristic_clearance(1.0)
    assert zero.heuristic_clearance == 1.0
    changed = yardstick(zero, starts, goals, seeds)
    zero.set_heuristic_clearance(0.0)
    assert zero.heuristic_clearance == 0.0
    got = yardstick(zero, starts, goals, seeds)
    assert any(not np.array_equal(a["expanded"], b["expanded"]) for a, b in zip(changed, want))  # (the detour through 1.0 was no no-op)
    for q, (a, b) in enumerate(zip(got, want)):
        for k in ("status", "n_expanded", "n_nodes", "n_path", "n_rng_draws", "n_rs_attempts", "n_state_checks", "n_path_checks", "n_lattice_boundary_hits"):
            assert a[k] == b[k], (q, k)
        assert a["cost"] == b["cost"] or (math.isnan(a["cost"]) and math.isnan(b["cost"])), q
        assert np.array_equal(a["expanded"], b["expanded"]), q
        for k in ("poses", "kind", "prim", "length"):
            assert np.array_equal(a["path"][k], b["path"][k]), (q, k)
        assert np.array_equal(zero.get_obstacle_field_of(q).view(np.uint32), plain.get_obstacle_field_of(q).view(np.uint32)), q


# ------------------------------------------------------------------------------------ 3: the views follow the map --
def _three_goal_fields(w, occ, d2, radius, goals):
    ow = inflate(O.World(lower=tuple(w.lb[:2]), upper=tuple(w.ub[:2]), resolution=RES), radius, occ=occ, d2=d2)
    return [ow.obstacle_heuristic(g[:2])[0] for g in goals]


def _map_edit_steps(w, ms):
    """yields (occupancy, d2) as the device map holds them after: nothing, an occupancy edit (pp_map_rasterize_segments), a new distance grid
    (pp_map_upload_dist2)"""
    yield "initial", w.occ(), w.d2()
    pose = [0.3 * w.ub[0], -0.35 * w.ub[1], 0.4]
    ident = w.add_rectangle(3.0, 1.0, pose)  # (the oracle's occupancy changes at once, its distance grid only with update())
    assert ms.add_polygon(rect_vertices(3.0, 1.0), pose, ident) > 0
    assert np.array_equal(ms.download_occupancy(), w.occ())
    yield "occupancy edit", w.occ(), w.d2()
    w.update()
    ms.upload_dist2(w.d2())
    yield "new distance grid", w.occ(), w.d2()


def test_views_follow_the_map_planner():
    """a planner keeps its views between batches: after every writer of either grid the next batch's fields are the oracle's of the NEW pair,
    which differ from the fields of the pair before (so reusing the old views fails)"""
    import pathplanning_amd as pa
    grid, radius = FIELD_GRIDS[1], 1.0
    w, ms, ctx = device_grid(grid, path_cost=True)
    val = pa.StateValidatorOccupancyMap(ms)
    planner = pa.HybridAStarBatch(val, max_batch=3, max_nodes=1024)
    planner.initialize()
    planner.set_heuristic_clearance(radius)
    goals = np.array([[-8.0, -14.0, 0.0], [8.5, 14.5, 1.0], [0.0, 0.0, -1.0]])
    starts = goals[::-1].copy()
    before = None
    for step, occ, d2 in _map_edit_steps(w, ms):
        planner.search_batch(starts, goals, [1, 2, 3])
        want = _three_goal_fields(w, occ, d2, radius, goals)
        for q in range(3):
            assert np.array_equal(planner.get_obstacle_field_of(q).view(np.uint32), want[q].view(np.uint32)), (step, q)
        if before is not None:
            assert all(not np.array_equal(a, b) for a, b in zip(before, want)), step
        before = want


def test_views_follow_the_map_pipeline():
    """the same through a pipeline: the guard at submission rebuilds the views when either map version has moved"""
    import pathplanning_amd as pa
    grid, radius = FIELD_GRIDS[1], 1.0
    w, ms, ctx = device_grid(grid, path_cost=True)
    val = pa.StateValidatorOccupancyMap(ms)
    pipe = pa.HybridAStarPipeline(val, capacity=8, max_nodes=1024, search_rows=4)
    pipe.initialize()
    pipe.set_heuristic_clearance(radius)
    assert pipe.heuristic_clearance == radius
    goals = np.array([[-8.0, -14.0, 0.0], [8.5, 14.5, 1.0], [0.0, 0.0, -1.0]])
    starts = goals[::-1].copy()
    seeds = np.array([1, 2, 3], dtype=np.uint64)
    before = None
    for step, occ, d2 in _map_edit_steps(w, ms):
        want = _three_goal_fields(w, occ, d2, radius, goals)
        seen = []
        run_pipe(pipe, starts, goals, seeds, chunk=3, hold=False,
                 inspect=lambda q, t, r: seen.append((q, np.array_equal(pipe.get_obstacle_field_of(t).view(np.uint32), want[q].view(np.uint32)))))
        assert sorted(seen) == [(0, True), (1, True), (2, True)], (step, seen)
        if before is not None:
            assert all(not np.array_equal(a, b) for a, b in zip(before, want)), step
        before = want
    pipe.close()


# ------------------------------------------------------------------------------------- 4: two radii on one map --
def test_two_planners_with_different_radii_share_a_map():
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    rng = np.random.RandomState(41)
    n = 6
    planners, oracles = {}, {}
    table = None
    for radius in RADII:
        p = pa.HybridAStarBatch(val, max_batch=n, max_nodes=32768)
        p.initialize(table)
        table = p.nonholo_table()
        p.set_heuristic_clearance(radius)
        planners[radius] = p
        ow = inflate(O.synthetic_world(256, 6, 3), radius)
        oracles[radius] = (ow, O.Hybrid(ow, table=table))
    for rnd in range(2):  # 0.35, 1.0, 0.35, 1.0
        starts, goals = valid_random_poses(rng, w, n), valid_random_poses(rng, w, n)
        seeds = np.arange(n, dtype=np.uint64) + 10 * rnd
        for radius in RADII:
            p, (ow, h) = planners[radius], oracles[radius]
            res = p.search_batch(starts, goals, seeds)
            compare(p, res, h, starts, goals, seeds)
            for q in (0, n - 1):
                assert np.array_equal(p.get_obstacle_field_of(q).view(np.uint32), ow.obstacle_heuristic(goals[q][:2])[0].view(np.uint32)), (rnd, radius, q)


# ---------------------------------------------------------------------------------------------- 5: the searches --
N_SEARCH = 24


def _search_world():
    w = O.synthetic_world(256, 14, 3)
    w.set_validator(1.0, 0.1)
    return w


@functools.lru_cache(maxsize=None)
def search_case():
    """the map and the 24 queries: valid random poses 2i (start) and 2i + 1 (goal) of RandomState(7), seed i; the oracle WITH the inflated
    occupancy (whole results) and WITHOUT it (expansion counts)"""
    w = _search_world()
    half = 256 * RES / 2
    rng = np.random.RandomState(7)
    qs = []
    while len(qs) < 2 * N_SEARCH:
        p = np.array([rng.uniform(-half + 1.5, half - 1.5), rng.uniform(-half + 1.5, half - 1.5), rng.uniform(-3.1, 3.1)])
        if w.is_state_valid(p[None])[0]:
            qs.append(p)
    starts, goals = np.array(qs[0::2]), np.array(qs[1::2])
    seeds = np.arange(N_SEARCH, dtype=np.uint64)
    table, _ = O.nonholo_build(w.lb, w.ub, O.params_array())
    _, _, _, plain_expansions = O.hybrid_batch(w, table, starts, goals, seeds, threads=8)
    wi = inflate(_search_world(), 1.0)
    h = O.Hybrid(wi, table=table)
    inflated = [h.search(starts[i], goals[i], int(seeds[i])) for i in range(N_SEARCH)]
    return starts, goals, seeds, table, np.asarray(plain_expansions), inflated, h


class _Replay:
    """Hybrid.search's interface over results computed once (test_gpu_hybrid.compare and test_gpu_pipeline.check_against_oracle ask per query)"""

    def __init__(self, starts, goals, seeds, results):
        self.key = {(tuple(starts[i]), tuple(goals[i]), int(seeds[i])): results[i] for i in range(len(results))}

    def search(self, start, goal, seed=0):
        return self.key[(tuple(start), tuple(goal), int(seed))]


def test_the_clearance_changes_the_oracle_searches():
    """keeps the comparisons below from passing on a no-op: at least 12 of the 24 expansion counts differ between the two rules (16 when this
    was written; 17 expansion sequences differ), and the clearance's sum is the smaller one (2 574 against 10 114)"""
    _, _, _, _, plain, inflated, _ = search_case()
    with_clearance = np.array([len(r["expanded"]) for r in inflated])
    print("expansions plain", int(plain.sum()), "clearance", int(with_clearance.sum()), "differ", int((plain != with_clearance).sum()))
    assert (plain != with_clearance).sum() >= 12
    assert with_clearance.sum() < plain.sum()


def _search_map():
    import pathplanning_amd as pa
    w = _search_world()
    ctx = pa.Context(0)
    ms = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, RES)
    ms.upload_dist2(w.d2())
    ms.upload_occupancy(w.occ())
    ms.upload_path_cost(w.pathcost())
    val = pa.StateValidatorOccupancyMap(ms)
    assert val.min_safe_radius == 1.0
    return w, ms, val, ctx


@pytest.mark.parametrize("rows_kernel", ["0", "1"])
def test_batch_searches_equal_the_oracle(monkeypatch, rows_kernel):
    """the one-wave planner and the rows planner (forced with PP_SEARCH_ROWS, as tests/test_gpu_hybrid.py does): all 24 queries, status,
    expansion sequence, node / RNG / check counters exactly, cost and path within 1e-5"""
    import pathplanning_amd as pa
    monkeypatch.setenv("PP_SEARCH_ROWS", rows_kernel)
    starts, goals, seeds, table, plain, inflated, _ = search_case()
    w, ms, val, ctx = _search_map()
    planner = pa.HybridAStarBatch(val, max_batch=N_SEARCH, max_nodes=32768, search_rows=8 if rows_kernel == "1" else 0)
    assert (planner.search_rows > 0) == (rows_kernel == "1")
    planner.initialize(table)
    planner.set_heuristic_clearance(1.0)
    res = planner.search_batch(starts, goals, seeds)
    n_ok = compare(planner, res, _Replay(starts, goals, seeds, inflated), starts, goals, seeds)
    assert n_ok == sum(r["status"] == 0 for r in inflated) == N_SEARCH  # (the query the plain rule fails on is solved)
    assert sum(r.n_expanded for r in res) < plain.sum()


def test_pipeline_searches_equal_the_oracle():
    import pathplanning_amd as pa
    starts, goals, seeds, table, plain, inflated, _ = search_case()
    w, ms, val, ctx = _search_map()
    pipe = pa.HybridAStarPipeline(val, capacity=8, max_nodes=32768, search_rows=8, log_expansions=True)  # every slot is recycled three times
    pipe.initialize(table)
    pipe.set_heuristic_clearance(1.0)
    replay = _Replay(starts, goals, seeds, inflated)
    checked = []
    rec, _ = run_pipe(pipe, starts, goals, seeds, chunk=5, logged=True,
                      inspect=lambda q, t, r: checked.append((q, check_against_oracle(pipe, t, r, replay, starts[q], goals[q], seeds[q]))))
    assert sorted(q for q, _ in checked) == list(range(N_SEARCH)) and all(ok for _, ok in checked)
    for q, r in enumerate(rec):
        assert r["n_lattice_boundary_hits"] == inflated[q]["n_lattice_boundary_hits"], q
    pipe.close()


# ------------------------------------------------------------------------------------------ 6: with a footprint --
def test_with_a_footprint_the_pipeline_is_the_one_wave_planner():
    """CAR3 has no disc on the reference point, so the clearance is the point disc's radius, minSafeRadius: the pipeline with footprint and
    clearance equals the one-wave footprint planner with the same clearance, query by query (tests/test_gpu_pipeline_footprint.py's list)"""
    import pathplanning_amd as pa
    assert all((ox, oy) != (0.0, 0.0) for ox, oy, _ in R.CAR3)
    w, ms, val, ctx = make_pair(256, 6, 3)
    g = R.Grid(w)
    radius = val.min_safe_radius
    rng = np.random.RandomState(346)
    n = 24
    starts, goals = R.valid_poses(rng, g, w, n, R.CAR3), R.valid_poses(rng, g, w, n, R.CAR3)
    seeds = np.arange(n, dtype=np.uint64) + 900
    planner = pa.HybridAStarBatch(val, max_batch=n, max_nodes=65536)
    assert planner.search_rows == 0
    planner.initialize()
    fp = pa.Footprint(ms, R.CAR3)
    planner.set_footprint(fp)
    without = yardstick(planner, starts, goals, seeds)
    planner.set_heuristic_clearance(radius)
    want = yardstick(planner, starts, goals, seeds)
    assert any(a["n_expanded"] != b["n_expanded"] for a, b in zip(without, want))
    pipe = pa.HybridAStarPipeline(val, capacity=8, max_nodes=65536, search_rows=8, log_expansions=True)
    pipe.initialize(planner.nonholo_table())
    pipe.set_footprint(fp)
    pipe.set_heuristic_clearance(radius)
    got, _ = run_pipe(pipe, starts, goals, seeds, chunk=5, logged=True)
    assert sum(c["status"] == 0 for c in got) >= n // 2
    for q in range(n):
        assert_is_the_one_wave_search(got[q], want[q], q)
    pipe.close()


def test_with_a_footprint_the_planners_fields_are_test_ones():
    """the one-wave footprint planner's fields for three of test 1's goals (the near-obstacle one among them) are test 1's oracle fields"""
    import pathplanning_amd as pa
    grid, radius = FIELD_GRIDS[1], 1.0
    w, ms, ctx = device_grid(grid, path_cost=True)
    val = pa.StateValidatorOccupancyMap(ms)
    planner = pa.HybridAStarBatch(val, max_batch=3, max_nodes=1024)
    planner.initialize()
    planner.set_footprint(pa.Footprint(ms, R.CAR3))
    planner.set_heuristic_clearance(radius)
    picks = (4, 7, 20)
    goals = np.array([list(field_goals(grid, radius)[i]) + [0.5] for i in picks])
    planner.search_batch(goals[::-1].copy(), goals, [1, 2, 3])
    for q, i in enumerate(picks):
        assert np.array_equal(planner.get_obstacle_field_of(q).view(np.uint32), oracle_fields(grid, radius)[i].view(np.uint32)), i


# ---------------------------------------------------------------------------------------------------- 7: rules --
def test_rules():
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError, ptr
    w, ms, val, ctx = make_pair(256, 6, 3)
    heur = pa.ObstaclesHeuristic(ms)
    planner = pa.HybridAStarBatch(val, max_batch=2, max_nodes=1024)
    pipe = pa.HybridAStarPipeline(val, capacity=8, max_nodes=32768, search_rows=4)
    pipe.initialize()
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        for call in (lambda: heur.update([(0.0, 0.0)], clearance=bad), lambda: planner.set_heuristic_clearance(bad), lambda: pipe.set_heuristic_clearance(bad)):
            with pytest.raises(PPError) as e:
                call()
            assert e.value.code == PP_ERR_INVALID and "clearance" in str(e.value), bad
    assert planner.heuristic_clearance == 0.0 and pipe.heuristic_clearance == 0.0
    # a pipeline's buffer set takes its radius from the pipeline
    assert ms.lib.pp_planner_set_heuristic_clearance(pipe.planner_h, C.c_float(0.5)) == PP_ERR_INVALID
    assert b"pp_pipeline_set_heuristic_clearance" in ms.lib.pp_last_error()
    # a map without a distance grid
    ms2 = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, RES)
    ms2.upload_occupancy(w.occ())
    with pytest.raises(PPError) as e:
        pa.ObstaclesHeuristic(ms2).update([(0.0, 0.0)], clearance=0.5)
    assert e.value.code == PP_ERR_INVALID and "distance grid" in str(e.value)
    # in flight: the footprint rule's error and message
    rng = np.random.RandomState(5)
    starts, goals = valid_random_poses(rng, w, 8), valid_random_poses(rng, w, 8)
    tickets = pipe.submit(starts, goals, np.arange(8, dtype=np.uint64))
    assert len(tickets) == 8 and pipe.in_flight() == 8
    with pytest.raises(PPError) as e:
        pipe.set_heuristic_clearance(1.0)
    assert e.value.code == PP_ERR_INVALID and "8 queries in flight: poll them all before changing" in str(e.value)
    with pytest.raises(PPError) as e2:
        pipe.set_footprint(pa.Footprint(ms, R.CAR3))
    assert e2.value.code == e.value.code and "8 queries in flight: poll them all before changing" in str(e2.value)
    assert pipe.heuristic_clearance == 0.0
    done = 0
    import time
    t0 = time.time()
    while done < 8:
        t, _ = pipe.poll(8, release=True)
        done += len(t)
        assert time.time() - t0 < 60
    pipe.set_heuristic_clearance(1.0)  # nothing in flight: accepted
    assert pipe.heuristic_clearance == 1.0
    pipe.close()


# ------------------------------------------------------------------------------------- the C++ mirror / pyplanning --
def test_pyplanning_hands_the_clearance_on():
    """HybridAStar::SetHeuristicClearance through the pybind11 module: the 24 queries with clearance 1.0 are the oracle's on the inflated
    occupancy (status, expansion count, cost), and after set_heuristic_clearance(0) the plain oracle's expansion counts"""
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "pathplanning_amd", "lib"))
    nav = importlib.import_module("pyplanning")
    starts, goals, seeds, table, plain, inflated, _ = search_case()
    w = _search_world()
    ss = nav.StateSpaceSE2(nav.Pose2d(*w.lb), nav.Pose2d(*w.ub))
    m = nav.OccupancyMap(0.1)
    val = nav.StateValidatorOccupancyMap(ss, m)
    m.set_grids(w.occ(), w.d2(), w.pathcost())
    algo = nav.HybridAStar(nav.HybridAStarSearchParameters(), N_SEARCH)
    assert algo.heuristic_clearance == 0.0
    algo.set_heuristic_clearance(1.0)
    assert algo.initialize(val) and algo.heuristic_clearance == 1.0
    res = algo.search_batch(starts, goals, seeds)
    for q, (status, cost, n_expanded, n_path) in enumerate(res):
        r = inflated[q]
        assert (status, n_expanded, n_path) == (r["status"], len(r["expanded"]), len(r["path_poses"])), q
        assert abs(cost - r["cost"]) < 1e-5, q
    algo.set_heuristic_clearance(0.0)
    res = algo.search_batch(starts, goals, seeds)
    assert [r[2] for r in res] == [int(x) for x in plain]
