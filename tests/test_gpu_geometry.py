"""-m gpu: the device against the CPU oracle off the default geometry -- non-square grids, cell sizes other than 0.1 m, a state box
that is not centred on the grid, and search lattices / vehicles other than the defaults.

Every other parity test runs on square maps of 0.1 m cells centred on the origin with the default lattice, where a swapped row / column
index, the LDS distance window's fall-back, the even-na chunk stride of the negative-k table read, or a state box read in place of the
grid's extent (or the reverse) would all go unnoticed.  Each world and parameter set below asserts the property that makes it reach
its code path before comparing anything."""
import math
import time

import numpy as np
import pytest

import oracle_lib as O
from gpu_common import box_random_poses, box_valid_random_poses, make_pair, make_pair_bounds
from test_gpu_hybrid import compare, run_pair

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-5

# dims: the grid the sizing code gives (ceil of the float extent over the float cell); branch: the kernel launch_check_states picks for
# an aligned batch of >= 2^20 poses (see check_states_branch)
WORLDS = {
    # rows != cols, neither a multiple of 64; ceil(cells / 64) odd: large batches take the pipelined kernel, not the LDS-bitmap one
    "A": dict(lower=(-16.65, -10.0), upper=(16.65, 10.0), res=0.1, dims=(333, 200), branch="pipe", params=("P1", "P3"), obstacles=10, seed=1),
    # 0.05 m cells: 1.5 m arcs span 30 cells, past the 16-cell distance window; the LDS-bitmap kernel on a non-square grid
    "B": dict(lower=(-11.2, -8.0), upper=(11.2, 8.0), res=0.05, dims=(448, 320), branch="lds", params=("P0", "P5"), obstacles=8, seed=2),
    # 0.15 m cells (inexact in float): the reciprocal-based cell division at a cell size that is not a power of two
    "C": dict(lower=(-12.15, -15.0), upper=(12.15, 15.0), res=0.15, dims=(162, 200), branch="pipe", params=("P2",), obstacles=10, seed=3),
    # state box != grid extent: the grid is centred on the local origin whatever the box (occupancy_map.cpp:6-14)
    "D": dict(lower=(-7.3, -20.1), upper=(18.9, 4.4), res=0.1, dims=(262, 245), branch="pipe", params=("P4",), obstacles=10, seed=4),
}

PARAMS = {
    "P0": {},
    "P1": dict(min_turning_radius=4.0, wheelbase=3.1, forward_cost_multiplier=1.5),
    "P2": dict(spatial_resolution=0.5, angular_resolution=0.0436),
    "P3": dict(spatial_resolution=2.0, angular_resolution=0.0875),
    "P4": dict(forward_cost_multiplier=0.7, reverse_cost_multiplier=1.0, voronoi_cost_multiplier=0.0, direction_switching_cost=2.0),
    "P5": dict(min_turning_radius=1.0),
}

COMBOS = [(wn, pn) for wn, spec in WORLDS.items() for pn in spec["params"]]
assert {pn for _, pn in COMBOS} == set(PARAMS) and {wn for wn, _ in COMBOS} == set(WORLDS)

_ENVS = {}


def env(name):
    """(world, map set, validator, context) of a world, built once per module"""
    if name not in _ENVS:
        spec = WORLDS[name]
        _ENVS[name] = make_pair_bounds(spec["lower"], spec["upper"], spec["res"], spec["obstacles"], spec["seed"])
        w = _ENVS[name][0]
        assert (w.rows, w.cols) == spec["dims"], (name, w.rows, w.cols)
    return _ENVS[name]


def param(name, key):
    return {**O.DEFAULT_PARAMS, **PARAMS[name]}[key]


def arc_cells(pn, res):
    """the search's arc length (1.5 x the spatial resolution, hybrid_a_star.cpp) in cells"""
    return 1.5 * param(pn, "spatial_resolution") / res


def table_na(pn):
    return int(math.ceil(2 * math.pi / param(pn, "angular_resolution")))  # heuristics.cpp:13


def check_states_branch(rows, cols, n, aligned):
    """the kernel launch_check_states (pp_kernels_basic.hip) runs for the head of an n-pose batch: "lds" (validity bitmap in LDS: fits
    in 128 KiB and ceil(cells / 64) even), "pipe" (>= 64 tiles of 1024 poses) or "staged" (small batches, misaligned views, the tail)"""
    words = ((rows * cols + 63) // 64) * 2
    if aligned and words * 4 <= 128 * 1024 and words % 4 == 0 and n >= (1 << 20):
        return "lds"
    if aligned and n >= 64 * 1024:
        return "pipe"
    return "staged"


def edge_poses(w, rng):
    """poses exactly on the state bounds and on cell boundaries (origin + k * res), and one ulp either side of each"""
    res = float(w.resolution)
    lo = np.maximum(w.lb[:2], w.grid_lo)
    hi = np.minimum(w.ub[:2], w.grid_hi)
    out = []

    def around(v):
        return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]

    def add(axis, values):
        for v in values:
            for vv in around(v):
                p = np.array([rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1]), rng.uniform(-math.pi, math.pi)])
                p[axis] = vv
                out.append(p)

    for axis in (0, 1):
        add(axis, [w.lb[axis], w.ub[axis]])
        n = (w.rows, w.cols)[axis]
        ks = sorted(set([0, 1, 2, n // 3, n // 2, n - 2, n - 1, n, n + 1] + list(rng.randint(0, n, 24))))
        add(axis, [w.grid_lo[axis] + k * res for k in ks])
    for t in (math.pi, -math.pi):  # heading bounds
        for tt in around(t):
            out.append(np.array([rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1]), tt]))
    for x, y in ((w.lb[0], w.lb[1]), (w.lb[0], w.ub[1]), (w.ub[0], w.lb[1]), (w.ub[0], w.ub[1]),
                 (w.grid_lo[0], w.grid_lo[1]), (w.grid_hi[0], w.grid_hi[1])):  # corners of the box and of the grid
        for xx in around(x):
            for yy in around(y):
                out.append(np.array([xx, yy, 0.0]))
    return np.array(out)


def mismatch_poses(w, rng, n):
    """(inside the box but off the grid, inside the grid but outside the box) -- both empty when the two coincide"""
    p = box_random_poses(rng, w, 40 * n, margin=0.0)
    p[:, 2] = rng.uniform(-math.pi, math.pi, len(p))
    in_box = (p[:, 0] >= w.lb[0]) & (p[:, 0] <= w.ub[0]) & (p[:, 1] >= w.lb[1]) & (p[:, 1] <= w.ub[1])
    in_grid = (p[:, 0] >= w.grid_lo[0]) & (p[:, 0] < w.grid_hi[0]) & (p[:, 1] >= w.grid_lo[1]) & (p[:, 1] < w.grid_hi[1])
    return p[in_box & ~in_grid][:n], p[in_grid & ~in_box][:n]


def state_cases(name, rng):
    w = env(name)[0]
    cases = [edge_poses(w, rng)]
    box_only, grid_only = mismatch_poses(w, rng, 200)
    if name == "D":
        assert len(box_only) == 200 and len(grid_only) == 200
        assert not w.is_state_valid(box_only).any() and not w.is_state_valid(grid_only).any()
        cases += [box_only, grid_only]
    return np.concatenate(cases)


@pytest.mark.parametrize("name", list(WORLDS))
def test_world_geometry_and_dispatch(name):
    """the preconditions every other test of this file stands on"""
    w, ms, val, ctx = env(name)
    spec = WORLDS[name]
    assert check_states_branch(w.rows, w.cols, 1 << 20, True) == spec["branch"]
    assert check_states_branch(w.rows, w.cols, (1 << 16) + 77, True) == "pipe"
    assert check_states_branch(w.rows, w.cols, (1 << 20) + 1237, False) == "staged"
    if name == "A":
        assert w.rows != w.cols and w.rows % 64 and w.cols % 64 and ((w.rows * w.cols + 63) // 64) % 2 == 1
    if name == "B":
        assert w.rows != w.cols and arc_cells("P0", float(w.resolution)) > 16
    if name == "D":
        assert not np.allclose(w.grid_lo, w.lb[:2]) and not np.allclose(w.grid_hi, w.ub[:2])
        assert np.array_equal(ms.grid_origin, w.origin)
    occ = w.occ() >= 0
    assert 0.001 < occ.mean() < 0.1  # obstacles inside the grid


@pytest.mark.parametrize("name", list(WORLDS))
def test_check_states_every_kernel(name):
    """is_state_valid bit-exact on random poses, bounds and cell boundaries +- 1 ulp, and (world D) poses in the box but off the grid and
    the reverse -- through the kernel each batch size selects, and through the staged kernel on a misaligned view"""
    import torch
    w, ms, val, ctx = env(name)
    rng = np.random.RandomState(100 + ord(name))
    extra = state_cases(name, rng)
    for n in ((1 << 20) + 1237, (1 << 16) + 77, 3000 + len(extra)):
        poses = box_random_poses(rng, w, n)
        for at in (0, n // 2, n - len(extra)):
            poses[at:at + len(extra)] = extra
        want = w.is_state_valid(poses).astype(bool)
        assert 0.05 < want.mean() < 0.95
        t = torch.from_numpy(poses).cuda()
        assert t.data_ptr() % 16 == 0
        out = val.is_state_valid(t)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy().astype(bool), want), (name, n, "aligned")
        buf = torch.from_numpy(np.concatenate([[0.0], poses.reshape(-1)])).cuda()
        view = buf[1:]  # 8-byte offset: the staged kernel, element by element
        assert view.data_ptr() % 16 == 8
        out = val.is_state_valid(view)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy().astype(bool), want), (name, n, "misaligned")
    assert np.array_equal(val.is_state_valid(extra), w.is_state_valid(extra).astype(bool))


@pytest.mark.parametrize("name", list(WORLDS))
def test_check_arcs_and_segments(name):
    """IsPathValid over constant-steer arcs (validity and last-valid ratio) of each parameter set the world is searched with, arc lengths
    including the search's 1.5 x spatial resolution, and over R2 segments: bit-exact"""
    import pathplanning_amd as pa
    w, ms, val, ctx = env(name)
    rng = np.random.RandomState(200 + ord(name))
    n = 30000
    for pn in WORLDS[name]["params"]:
        P = pa.HybridAStarSearchParameters(num_generated_motion=9, **PARAMS[pn])
        steer, curv, direc = P.primitives()
        frm = box_valid_random_poses(rng, w, n)
        frm[: n // 10] = box_random_poses(rng, w, n // 10)  # some starts invalid (ratio 0), some off the grid or the box
        pick = rng.randint(0, len(steer), n)
        arc = 1.5 * P.spatial_resolution
        length = rng.choice([arc, 0.0, 3.0, 7.5], n, p=[0.7, 0.02, 0.18, 0.1])
        v_got, l_got = val.is_path_valid(frm, curv[pick], length, direc[pick])
        v_want, l_want = w.is_path_valid_csteer(frm, steer[pick], length, direc[pick], wheelbase=P.wheelbase)
        assert np.array_equal(v_got, v_want.astype(bool)), (name, pn)
        assert np.array_equal(l_got, l_want), (name, pn)
        assert 0.02 < (~v_got).mean() < 0.9
    a = box_valid_random_poses(rng, w, n)[:, :2]
    b = a + rng.uniform(-4, 4, (n, 2))
    b[:50] = a[:50]  # zero-length paths
    got = val.is_segment_valid(a, b)
    want = w.is_path_valid_r2(a, b).astype(bool)
    assert np.array_equal(got, want)
    assert 0.02 < (~want).mean() < 0.9


@pytest.mark.parametrize("name", list(WORLDS))
def test_rollout_children(name):
    """GetConstantSteerChild for parents x primitives with the world's first parameter set: validity and discrete keys bit-exact,
    poses / costs / lengths within 1e-5"""
    import ctypes as C
    import pathplanning_amd as pa
    from pathplanning_amd._lib import check, ptr
    w, ms, val, ctx = env(name)
    pn = WORLDS[name]["params"][0]
    P = pa.HybridAStarSearchParameters(**PARAMS[pn])
    steer, curv, direc = P.primitives()
    h = O.Hybrid(w, O.params_array(**PARAMS[pn]))
    assert h.P == len(curv)
    rng = np.random.RandomState(300 + ord(name))
    parents = box_valid_random_poses(rng, w, 3000)
    parents[:, 2] += rng.choice([0.0, 2 * math.pi, -2 * math.pi], len(parents), p=[0.8, 0.1, 0.1])
    want = h.children(parents)
    n, Pn = len(parents), len(curv)
    valid = np.empty((n, Pn), dtype=np.uint8)
    pose = np.empty((n, Pn, 3))
    key = np.empty((n, Pn, 3), dtype=np.int32)
    cost = np.empty((n, Pn))
    length = np.empty((n, Pn))
    cp = P.to_c()
    check(ms.lib.pp_rollout_children(ms.h, C.byref(cp), Pn, ptr(curv), ptr(direc), n, ptr(np.ascontiguousarray(parents)), ptr(valid), ptr(pose),
                                     ptr(key), ptr(cost), ptr(length)))
    assert np.array_equal(valid, want["valid"])
    assert np.array_equal(key, want["keys"])
    assert np.abs(pose - want["poses"]).max() < POSE_TOL
    m = valid.astype(bool)
    assert np.abs(cost[m] - want["cost"][m]).max() < POSE_TOL
    assert np.abs(length[m] - want["length"][m]).max() < POSE_TOL
    assert 0.005 < 1 - m.mean() < 0.95


@pytest.mark.parametrize("name", list(WORLDS))
def test_distance_grid_at_the_world_resolution(name):
    """(float)(sqrt((double)d2) * resolution), gvd.h:38, with the world's own float cell size"""
    w, ms, val, ctx = env(name)
    d2 = w.d2()
    want = (np.sqrt(d2.astype(np.float64)) * np.float64(np.float32(WORLDS[name]["res"]))).astype(np.float32)
    got = ms.download_distance()
    assert got.shape == (w.rows, w.cols)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(WORLDS))
def test_obstacle_heuristic_fields(name):
    """ObstaclesHeuristic::Update for the grid's four corner cells, its centre, an occupied cell, a goal outside the grid (inside the box
    on world D) and a random one: bit-exact, explored set included"""
    import pathplanning_amd as pa
    w, ms, val, ctx = env(name)
    res = float(w.resolution)
    rng = np.random.RandomState(400 + ord(name))

    def centre_of(r, c):
        return (w.grid_lo[0] + (r + 0.5) * res, w.grid_lo[1] + (c + 0.5) * res)

    occupied = np.argwhere(w.occ() >= 0)
    r, c = occupied[len(occupied) // 2]
    goals = [centre_of(0, 0), centre_of(w.rows - 1, 0), centre_of(0, w.cols - 1), centre_of(w.rows - 1, w.cols - 1),
             centre_of(w.rows // 2, w.cols // 2), centre_of(r, c), tuple(box_valid_random_poses(rng, w, 1)[0, :2])]
    if name == "D":
        outside = (16.0, -5.0)  # in the box, beyond the grid's +x edge
        assert w.lb[0] <= outside[0] <= w.ub[0] and outside[0] > w.grid_hi[0]
    else:
        outside = (w.grid_hi[0] + 3.0, 0.0)
    goals.append(outside)
    assert w.to_cell([outside])[0].tolist() == [-1, -1]
    got = pa.ObstaclesHeuristic(ms).update(goals)
    n_explored = []
    for i, g in enumerate(goals):
        cost, explored = w.obstacle_heuristic(g)
        assert np.array_equal(got[i], cost), (name, i, g)
        assert np.array_equal(np.isfinite(got[i]), explored.astype(bool)), (name, i)
        n_explored.append(int(explored.sum()))
    assert n_explored[-1] == 0 and min(n_explored[:5] + n_explored[6:7]) > w.rows * w.cols // 2, n_explored


@pytest.mark.parametrize("wn,pn", COMBOS)
def test_nonholo_table(wn, pn):
    """NonHolonomicHeuristic::Build on the device for each parameter set a world is searched with: dims, offsets and values"""
    import pathplanning_amd as pa
    w, ms, val, ctx = env(wn)
    P = pa.HybridAStarSearchParameters(**PARAMS[pn])
    table, offs = pa.NonHolonomicHeuristic.build(ctx, w.lb, w.ub, P)
    want, offs_o = O.nonholo_build(w.lb, w.ub, O.params_array(**PARAMS[pn]))
    assert table.shape == want.shape
    assert table.shape[2] == table_na(pn)
    if wn == "A":
        assert table.shape[0] != table.shape[1]
    if pn == "P3":
        assert table.shape[2] % 2 == 0
    assert np.array_equal(offs, offs_o)
    diff = table != want
    assert diff.mean() < 1e-4, diff.mean()
    assert np.allclose(table, want, rtol=2e-7, atol=0)


def combo_queries(wn, pn):
    w = env(wn)[0]
    rng = np.random.RandomState(500 + 7 * ord(wn) + int(pn[1]))
    n = 12
    starts = box_valid_random_poses(rng, w, n)
    goals = box_valid_random_poses(rng, w, n)
    goals[0] = starts[0]  # start == goal
    if wn == "D":
        goals[1] = [16.0, -5.0, 0.0]  # inside the box, off the grid: the obstacle field stays +inf
        cand = box_valid_random_poses(rng, w, 400)  # along the two edges where box and grid part: the grid's +x edge, the box's +y edge
        starts[2], goals[2] = cand[np.argmax(cand[:, 0])], cand[np.argmax(cand[:, 1])]
        starts[3], goals[3] = cand[np.argmin(cand[:, 1])], cand[np.argmin(cand[:, 0])]
    seeds = np.arange(n, dtype=np.uint64) + 17 * int(pn[1]) + 1
    return starts, goals, seeds


def children_outside(w, h, pn, poses):
    """end poses of every primitive's full arc from `poses`: (inside the box but off the grid, inside the grid but outside the box)"""
    arc = 1.5 * param(pn, "spatial_resolution")
    d = h.deltas()
    ends = []
    for delta in d:
        for direction in (0, 1):
            ends.append(O.constant_steer(poses, delta, arc, direction, wheelbase=param(pn, "wheelbase")))
    e = np.concatenate(ends)
    in_box = (e[:, 0] >= w.lb[0]) & (e[:, 0] <= w.ub[0]) & (e[:, 1] >= w.lb[1]) & (e[:, 1] <= w.ub[1])
    in_grid = (e[:, 0] >= w.grid_lo[0]) & (e[:, 0] < w.grid_hi[0]) & (e[:, 1] >= w.grid_lo[1]) & (e[:, 1] < w.grid_hi[1])
    return int((in_box & ~in_grid).sum()), int((in_grid & ~in_box).sum())


@pytest.mark.parametrize("rows_kernel", ["0", "1"])
@pytest.mark.parametrize("wn,pn", COMBOS)
def test_batch_search(monkeypatch, wn, pn, rows_kernel):
    """12 queries per world and parameter set through both search kernels: status, expansion sequence, counters, path kinds and RS words
    exact; poses, cost and length within 1e-5"""
    monkeypatch.setenv("PP_SEARCH_ROWS", rows_kernel)
    w, ms, val, ctx = env(wn)
    res = float(w.resolution)
    starts, goals, seeds = combo_queries(wn, pn)
    if wn == "A":
        assert w.rows != w.cols
    if pn == "P3" or wn == "B":
        assert arc_cells(pn, res) > 16  # children's arcs leave the LDS distance window
    planner, results, h = run_pair(w, ms, val, PARAMS[pn], starts, goals, seeds, max_nodes=131072)
    nx, ny, na = planner.nonholo_table().shape
    assert na == table_na(pn)
    if wn == "A":
        assert nx != ny
    n_ok = compare(planner, results, h, starts, goals, seeds)
    assert n_ok >= 8, n_ok
    assert results[0].status == 0
    if pn == "P3":
        assert na % 2 == 0
        reads = [h.search(starts[q], goals[q], int(seeds[q]))["n_negative_k_stride_reads"] for q in range(len(starts))]
        assert sum(reads) > 0 and sum(1 for r in reads if r > 0) >= 4, reads
    if wn == "D":
        assert results[1].n_expanded > 10  # the off-grid goal (no obstacle field: the Euclidean heuristic) is searched for, not refused
        parents = np.concatenate([starts] + [planner.get_path_of(q)["poses"] for q in range(len(starts)) if results[q].status == 0])
        box_only, grid_only = children_outside(w, h, pn, parents)
        assert box_only > 0 and grid_only > 0, (box_only, grid_only)


def test_pipeline_on_the_off_centre_box():
    """the streaming pipeline on world D with P4 (forward cheaper than reverse, no Voronoi term, a switching cost): the batch planner's results"""
    import pathplanning_amd as pa
    w, ms, val, ctx = env("D")
    rng = np.random.RandomState(6)
    n = 240
    starts, goals = box_valid_random_poses(rng, w, n), box_valid_random_poses(rng, w, n)
    goals[5] = [16.0, -5.0, 0.0]
    seeds = np.arange(n, dtype=np.uint64) + 3
    P = pa.HybridAStarSearchParameters(**PARAMS["P4"])
    batch = pa.HybridAStarBatch(val, P, max_batch=n, max_nodes=65536, search_rows=64)
    batch.initialize()
    want = batch.search_batch(starts, goals, seeds)
    assert sum(r.status == 0 for r in want) >= n // 2
    pipe = pa.HybridAStarPipeline(val, P, capacity=64, max_nodes=65536, search_rows=32)  # every slot recycled
    pipe.initialize(batch.nonholo_table())
    fields = ("status", "n_expanded", "n_nodes", "n_path", "n_rng_draws", "n_rs_attempts", "n_state_checks", "n_path_checks", "n_lattice_boundary_hits")
    index_of, nxt, got = {}, 0, {}
    t0 = time.time()
    while len(got) < n:
        if nxt < n and pipe.free_slots() > 0:
            tickets = pipe.submit(starts[nxt:], goals[nxt:], seeds[nxt:])
            for i, t in enumerate(tickets):
                index_of[int(t)] = nxt + i
            nxt += len(tickets)
        tickets, res = pipe.poll(512)
        for i, t in enumerate(tickets):
            got[index_of[int(t)]] = res[i]
        if not len(tickets):
            time.sleep(0.0005)
        assert time.time() - t0 < 120
    for q, r in got.items():
        for f in fields:
            assert getattr(r, f) == getattr(want[q], f), (q, f, getattr(r, f), getattr(want[q], f))
        assert r.cost == want[q].cost or r.status != 0
    pipe.close()
    batch.close()


def test_rrt_on_the_off_centre_box():
    """RRT and RRT* sampling the asymmetric state box of world D (the grid covers only part of it): whole trees equal the oracle's"""
    import pathplanning_amd as pa
    from test_gpu_rrt import same_tree
    w, ms, val, ctx = env("D")
    lb, ub = w.lb[:2], w.ub[:2]
    init, goal = [-5.0, -10.0], [11.0, 2.0]
    assert ub[0] > w.grid_hi[0] and lb[1] < w.grid_lo[1]  # samples beyond the grid's +x and -y edges
    assert w.is_path_valid_r2([init], [init])[0] and w.is_path_valid_r2([goal], [goal])[0]
    for seed, star in ((1, True), (2, False)):
        cls = pa.RRTStar if star else pa.RRT
        r = cls(ctx, lb, ub, validator=val, max_iteration=4000, max_number_tree_node=4000, max_connection_distance=0.512, goal_bias=0.05)
        r.set_init_state(init)
        r.set_goal_state(goal)
        r.set_seed(seed)
        r.search_path()
        want = O.rrt(w, lb, ub, init, goal, seed, star=star, max_iteration=4000, max_nodes=4000, max_connection=0.512, goal_bias=0.05)
        same_tree(r.result, want)
        assert len(want["nodes"]) > 100


def fused_poses(lb, ub, n, seed):
    """k_check_states_fused's poses: pose i = lb + (ub - lb) * u01(splitmix64(seed + 3i + c)), c = 0, 1, 2 for x, y, theta; double
    operations in the kernel's order (no contraction)"""
    i = np.arange(n, dtype=np.uint64)
    k = np.uint64(seed) + np.uint64(3) * i

    def splitmix64(x):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))

    def u01(h):
        return (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)

    out = np.empty((n, 3))
    with np.errstate(over="ignore"):
        for c in range(3):
            u = u01(splitmix64(k + np.uint64(c)))
            out[:, c] = lb[c] + (ub[c] - lb[c]) * u
    return out


def test_fused_generator_restatement():
    """the numpy restatement of splitmix64 against the first two outputs of Vigna's splitmix64.c seeded with 1234567 (the kernel's
    splitmix64(s) is that generator's next() from state s; s + 3 for pose 1)"""
    p = fused_poses(np.zeros(3), np.full(3, 9007199254740992.0), 2, 1234567)  # u01 * 2^53 = the output's top 53 bits, exactly
    assert int(p[0, 0]) == 6457827717110365317 >> 11
    q = fused_poses(np.zeros(3), np.full(3, 9007199254740992.0), 1, 1234567 + 0x9E3779B97F4A7C15 - 1)
    assert int(q[0, 1]) == 3203168211198807973 >> 11


@pytest.mark.parametrize("name", ["A", "256"])
def test_fused_count(name):
    """pp_check_states_fused_dev: in-kernel poses, only a count leaves -- equal to the oracle's count of valid poses among the same ones"""
    import torch
    if name == "256":
        w, ms, val, ctx = make_pair(256, 6, 3)
    else:
        w, ms, val, ctx = env(name)
    n = (1 << 22) + 12345
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    for seed in (7, 0xDEADBEEFCAFEF00D):
        poses = fused_poses(w.lb, w.ub, n, seed)
        want = int(w.is_state_valid(poses).sum())
        assert 0.05 * n < want < 0.99 * n
        val.count_valid_fused(n, seed, cnt)
        ctx.synchronize()
        assert int(cnt.item()) == want, (name, seed, int(cnt.item()), want)
