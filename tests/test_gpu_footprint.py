"""-m gpu: the vehicle footprint (include/pp_hip.h, "vehicle footprint") on the device.
  * the footprint {(0, 0, minSafeRadius)} IS the point validator: flags and `last` equal pp_check_states / arcs / rs_paths / se2_paths on
    every input, no exclusions; the search with it equals the search without, bit for bit;
  * real footprints equal the numpy restatement (tests/footprint_ref.py) outside its guard band (at most 0.1 % of a test's cases);
  * the footprint follows its map's distance grid; the search with a car footprint keeps every edge of its tree valid for the car;
  * misuse is PP_ERR_INVALID with a message."""
import math

import numpy as np
import pytest

import footprint_ref as R
import oracle_lib as O
from gpu_common import make_pair

pytestmark = pytest.mark.gpu

RMIN = 2.0  # HybridAStarSearchParameters().min_turning_radius


def footprints(pa, ms):
    return {"car3": pa.Footprint(ms, R.CAR3), "cover5": pa.Footprint.cover_rectangle(ms, 4.8, 2.0, 1.0, 5), "two_radii": pa.Footprint(ms, R.TWO_RADII)}


def assert_share(flags):
    assert 0.2 < flags.mean() < 0.95, flags.mean()  # both verdicts are exercised


def assert_equal_outside_guard(guard, *pairs):
    assert guard.mean() <= R.MAX_LEFT_OUT, guard.mean()
    keep = ~guard
    for got, want in pairs:
        assert np.array_equal(np.asarray(got)[keep], np.asarray(want)[keep]), int((np.asarray(got)[keep] != np.asarray(want)[keep]).sum())


def path_inputs(rng, w, n):
    """arcs (random continuous curvature within the default primitives' range), Reeds-Shepp pairs and SE2 pairs"""
    frm = R.continuous_poses(rng, w, n, margin=0.9)
    kappa = rng.uniform(-0.5, 0.5, n)
    kappa[rng.rand(n) < 0.2] = 0.0
    length = rng.choice([1.5, 0.0, 3.0, 7.5], n, p=[0.5, 0.02, 0.38, 0.1])
    to = frm.copy()
    to[:, :2] += rng.uniform(-5, 5, (n, 2))
    to[:, 2] = rng.uniform(-1.2 * math.pi, 1.2 * math.pi, n)
    return frm, kappa, length, to


# ------------------------------------------------------------------------------------------------ 5: degenerate --
@pytest.mark.parametrize("radius", [1.0, 0.35])
def test_point_disc_is_the_point_validator_exactly(radius):
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    val.min_safe_radius = radius
    fp = pa.Footprint(ms, [(0.0, 0.0, radius)])
    rng = np.random.RandomState(5)
    n = 200000 + 777
    poses = R.continuous_poses(rng, w, n, margin=1.3)  # incl. out-of-box poses
    poses[::97, 2] = rng.uniform(-40, 40, len(poses[::97]))  # headings far beyond +-pi
    poses[5::1013, 0] = np.nan
    poses[7::1013, 1] = np.nan
    poses[9::1013, 2] = np.nan
    poses[11::1013, 0] = np.inf
    got = val.is_state_valid(poses, footprint=fp)
    want = val.is_state_valid(poses)
    assert np.array_equal(got, want)
    assert 0.05 < want.mean() < 0.95
    flags, clear = val.is_state_valid(poses[:5000], footprint=fp, return_clearance=True)
    assert np.array_equal(flags, want[:5000])
    dist = ms.download_distance()
    g = R.Grid(w)
    r, c, _, _ = R.cell(g, poses[:5000, 0], poses[:5000, 1])
    d = dist[np.clip(r, 0, w.rows - 1), np.clip(c, 0, w.cols - 1)]
    assert np.array_equal(clear[flags], (d - np.float32(radius))[flags]) and (clear[~flags] == -1).all()
    m = 20000
    frm, kappa, length, to = path_inputs(rng, w, m)
    frm[::211, 2] += 30.0
    frm[3::499, 0] = np.nan
    for backward in (0, 1):
        v, l = val.is_path_valid(frm, kappa, length, backward, footprint=fp)
        v0, l0 = val.is_path_valid(frm, kappa, length, backward)
        assert np.array_equal(v, v0) and np.array_equal(l, l0, equal_nan=True)
    ok = np.isfinite(frm).all(axis=1)
    paths = pa.ReedsSheppPaths(ctx, min_turning_radius=RMIN).connect(frm[ok], to[ok])
    paths["start"][3::499, 0] = np.nan  # records with NaN coordinates, made by hand (connect is not asked to solve them)
    paths["start"][5::499, 1] = np.nan
    paths["start"][7::499, 2] = np.nan
    paths["length"][11::499] = np.nan
    v, l = val.is_rs_path_valid(paths, footprint=fp)
    v0, l0 = val.is_rs_path_valid(paths)
    assert np.array_equal(v, v0) and np.array_equal(l, l0, equal_nan=True)
    v, l = val.is_se2_path_valid(frm, to, footprint=fp)
    v0, l0 = val.is_se2_path_valid(frm, to)
    assert np.array_equal(v, v0) and np.array_equal(l, l0, equal_nan=True)


# ---------------------------------------------------------------------------------------------- 6: restatement --
@pytest.mark.parametrize("n_cells,n_obstacles,seed", [(256, 6, 3), (512, 12, 3)])
def test_footprints_match_the_restatement(n_cells, n_obstacles, seed):
    import pathplanning_amd as pa
    import torch
    w, ms, val, ctx = make_pair(n_cells, n_obstacles, seed)
    g = R.Grid(w)
    rng = np.random.RandomState(60 + n_cells)
    n = 200000 + 333  # (a ragged tail behind the streamed kernel's whole tiles)
    poses = R.continuous_poses(rng, w, n)
    frm, kappa, length, to = path_inputs(rng, w, 20000)
    rs_paths = pa.ReedsSheppPaths(ctx, min_turning_radius=RMIN).connect(frm, to)
    for name, fp in footprints(pa, ms).items():
        discs = fp.discs
        want, clear_want, _, guard = R.fp_state(g, poses, discs)
        print("%s on %d^2: valid share %.3f, %d poses in the guard band" % (name, n_cells, want.mean(), guard.sum()))
        assert_share(want)
        got = val.is_state_valid(poses, footprint=fp)
        assert_equal_outside_guard(guard, (got, want))
        got, clear = val.is_state_valid(poses, footprint=fp, return_clearance=True)
        assert_equal_outside_guard(guard, (got, want), (clear, np.where(want, clear_want, np.float32(-1))))
        # device tensors: the streamed kernel (16-byte aligned), the general kernel (a view 8 bytes off that alignment), n = 0
        t = torch.from_numpy(poses).cuda()
        assert t.data_ptr() % 16 == 0
        buf = torch.empty(3 * n + 1, dtype=torch.float64, device="cuda")
        odd = buf[1:]
        odd.copy_(t.view(-1))
        assert odd.data_ptr() % 16 == 8
        torch.cuda.synchronize()  # (the validator's stream is not torch's)
        for src in (t, odd):
            out = val.is_state_valid(src, footprint=fp)
            ctx.synchronize()
            assert_equal_outside_guard(guard, (out.cpu().numpy().astype(bool), want))
        assert val.is_state_valid(np.zeros((0, 3)), footprint=fp).shape == (0,)
        assert val.is_state_valid(t[:0], footprint=fp).numel() == 0
        ctx.synchronize()
        for backward in (0, 1):
            v_want, l_want, guard_a, samples = R.fp_arcs(g, frm, kappa, length, backward, discs)
            print("  arcs backward=%d: valid share %.3f, %.2f samples per arc, %d in the guard band" % (backward, v_want.mean(), samples.mean(), guard_a.sum()))
            assert_share(v_want)
            v, l = val.is_path_valid(frm, kappa, length, backward, footprint=fp)
            assert_equal_outside_guard(guard_a, (v, v_want), (l, l_want))
        v_want, l_want, guard_r, _ = R.fp_rs_paths(g, rs_paths, discs)
        assert_share(v_want)
        v, l = val.is_rs_path_valid(rs_paths, footprint=fp)
        assert_equal_outside_guard(guard_r, (v, v_want), (l, l_want))
        v_want, l_want, guard_s, _ = R.fp_se2_paths(g, frm, to, discs)
        assert_share(v_want)
        v, l = val.is_se2_path_valid(frm, to, footprint=fp)
        assert_equal_outside_guard(guard_s, (v, v_want), (l, l_want))


def test_large_batches_on_the_1024_map():
    """2^20 whole tiles + a ragged tail on the 1024^2 map (128 KiB of bitmap per radius): the streamed kernel and the general one, against the
    restatement for real footprints and, for the point disc, against pp_check_states_dev on the same device-resident poses (exactly)"""
    import pathplanning_amd as pa
    import torch
    w, ms, val, ctx = make_pair(1024, 24, 1)
    g = R.Grid(w)
    rng = np.random.RandomState(1024)
    n = (1 << 20) + 4321
    poses = R.continuous_poses(rng, w, n)
    hard = poses.copy()  # out-of-box poses, far-wrapped headings, NaN / inf coordinates
    hard[:, :2] *= 1.25
    hard[::97, 2] = rng.uniform(-40, 40, len(hard[::97]))
    hard[5::1013, 0] = np.nan
    hard[7::1013, 1] = np.nan
    hard[9::1013, 2] = np.nan
    hard[11::1013, 1] = np.inf
    th = torch.from_numpy(hard).cuda()
    torch.cuda.synchronize()
    for radius in (1.0, 0.35):
        val.min_safe_radius = radius
        got = val.is_state_valid(th, footprint=pa.Footprint(ms, [(0.0, 0.0, radius)]))
        want0 = val.is_state_valid(th)
        ctx.synchronize()
        assert torch.equal(got, want0) and 0.05 < want0.float().mean().item() < 0.95
    val.min_safe_radius = 1.0
    for fp in (pa.Footprint(ms, R.CAR3), pa.Footprint(ms, R.TWO_RADII)):  # one bitmap, two bitmaps
        want, _, _, guard = R.fp_state(g, poses, fp.discs)
        assert_share(want)
        t = torch.from_numpy(poses).cuda()
        assert t.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        out = val.is_state_valid(t, footprint=fp)
        ctx.synchronize()
        assert_equal_outside_guard(guard, (out.cpu().numpy().astype(bool), want))
        assert_equal_outside_guard(guard, (val.is_state_valid(poses, footprint=fp), want))


# ---------------------------------------------------------------------------------------- 7: follows the map --
def test_footprint_follows_the_map():
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    w2 = O.synthetic_world(256, 9, 8)
    fp = pa.Footprint(ms, R.CAR3)
    rng = np.random.RandomState(70)
    poses = R.continuous_poses(rng, w, 100000)
    frm, kappa, length, _ = path_inputs(rng, w, 5000)
    first = None
    for i, world in enumerate((w, w2, w)):
        if i > 0:
            ms.upload_dist2(world.d2())
        g = R.Grid(w, d2=world.d2())
        want, _, _, guard = R.fp_state(g, poses, fp.discs)
        assert_equal_outside_guard(guard, (val.is_state_valid(poses, footprint=fp), want))
        v_want, l_want, guard_a, _ = R.fp_arcs(g, frm, kappa, length, 0, fp.discs)
        v, l = val.is_path_valid(frm, kappa, length, 0, footprint=fp)
        assert_equal_outside_guard(guard_a, (v, v_want), (l, l_want))
        if i == 0:
            first = want
        elif i == 1:
            assert (want != first).mean() > 0.02  # the second grid really is another one
    # ... a distance grid built on the device from another occupancy grid
    ms.upload_occupancy(w2.occ())
    ms.update_gvd()
    g = R.Grid(w)
    g.dist = ms.download_distance()
    want, _, _, guard = R.fp_state(g, poses, fp.discs)
    assert (want != first).mean() > 0.02
    assert_equal_outside_guard(guard, (val.is_state_valid(poses, footprint=fp), want))
    # ... and a float grid uploaded directly
    dist = (R.Grid(w, d2=w2.d2()).dist * np.float32(0.5)).astype(np.float32)
    ms.upload_distance(dist)
    g = R.Grid(w)
    g.dist = dist
    want, _, _, guard = R.fp_state(g, poses, fp.discs)
    assert_equal_outside_guard(guard, (val.is_state_valid(poses, footprint=fp), want))


# ------------------------------------------------------------------------------------------------- 8, 9: search --
def plan(planner, starts, goals, seeds):
    res = planner.search_batch(starts, goals, seeds)
    out = []
    for q in range(len(starts)):
        r = res[q]
        out.append(dict(status=r.status, cost=r.cost, n_expanded=r.n_expanded, n_nodes=r.n_nodes, expanded=planner.get_expanded_of(q), path=planner.get_path_of(q)))
    return out


def tree_of(planner, q, n_nodes):
    from pathplanning_amd._lib import check, ptr
    parents, poses = np.zeros(n_nodes, np.int32), np.zeros((n_nodes, 3))
    action, length = np.zeros(n_nodes, np.int32), np.zeros(n_nodes)
    check(planner.lib.pp_planner_debug_nodes(planner.h, q, n_nodes, ptr(parents), ptr(poses), None, None))
    check(planner.lib.pp_planner_debug_node_actions(planner.h, q, n_nodes, ptr(action), ptr(length)))
    return parents, poses, action, length


def edges_valid(g, discs, curv, direc, parent_pose, goal, action, length):
    """restatement's verdict on the edges that leave `parent_pose`, created by `action`: a primitive index (the constant-steer arc over its stored
    length), or 1000 + word (the analytic expansion: the optimal Reeds-Shepp path from the parent to the query's goal) -> valid, guard"""
    n = len(action)
    valid, guard = np.ones(n, bool), np.zeros(n, bool)
    arc = action < 1000
    if arc.any():
        a = action[arc]
        valid[arc], _, guard[arc], _ = R.fp_arcs(g, parent_pose[arc], curv[a], length[arc], direc[a], discs)
    if (~arc).any():
        paths = O.rs_connect(parent_pose[~arc], np.broadcast_to(goal, (int((~arc).sum()), 3)), RMIN)
        valid[~arc], _, guard[~arc], _ = R.fp_rs_paths(g, paths, discs)
    return valid, guard


@pytest.mark.parametrize("n_cells,n_obstacles,seed", [(256, 6, 3), (512, 12, 3)])
def test_search_with_the_point_disc_is_the_search_without(n_cells, n_obstacles, seed):
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(n_cells, n_obstacles, seed)
    g = R.Grid(w)
    rng = np.random.RandomState(80 + n_cells)
    n = 32
    starts, goals = R.valid_poses(rng, g, w, n, R.CAR3), R.valid_poses(rng, g, w, n, R.CAR3)
    seeds = np.arange(n, dtype=np.uint64) + 500
    planner = pa.HybridAStarBatch(val, max_batch=n, max_nodes=65536)
    assert planner.search_rows == 0
    planner.initialize()
    base = plan(planner, starts, goals, seeds)
    planner.set_footprint(pa.Footprint(ms, [(0.0, 0.0, val.min_safe_radius)]))
    with_fp = plan(planner, starts, goals, seeds)
    planner.set_footprint(None)
    again = plan(planner, starts, goals, seeds)
    assert sum(b["status"] == 0 for b in base) >= n // 2
    for b, f, a in zip(base, with_fp, again):
        for other in (f, a):
            assert (b["status"], b["n_expanded"], b["n_nodes"]) == (other["status"], other["n_expanded"], other["n_nodes"])
            assert b["cost"] == other["cost"] or (math.isnan(b["cost"]) and math.isnan(other["cost"]))
            assert np.array_equal(b["expanded"], other["expanded"])
            for k in ("poses", "kind", "prim", "length", "tuv"):
                assert np.array_equal(b["path"][k], other["path"][k]), k


@pytest.mark.parametrize("n_cells,n_obstacles,seed", [(256, 6, 3), (512, 12, 3)])
def test_search_with_the_car_footprint(n_cells, n_obstacles, seed):
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(n_cells, n_obstacles, seed)
    g = R.Grid(w)
    discs = R.CAR3
    params = pa.HybridAStarSearchParameters()
    _, curv, direc = params.primitives()
    full = 1.5 * params.spatial_resolution  # hybrid_a_star.cpp:115
    rng = np.random.RandomState(90 + n_cells)
    n = 32
    planner = pa.HybridAStarBatch(val, params, max_batch=n, max_nodes=65536)
    planner.initialize()
    fp = pa.Footprint(ms, discs)
    changed, edges_checked, edges_left_out, successes = 0, 0, 0, 0
    for rnd in range(4):
        starts, goals = R.valid_poses(rng, g, w, n, discs), R.valid_poses(rng, g, w, n, discs)
        if rnd == 0:  # two starts that the point validator accepts and the car does not: no plan may come out
            cand = R.continuous_poses(rng, w, 4000, margin=0.95)
            cand[:, 2] = rng.uniform(-math.pi, math.pi, len(cand))
            car_ok, _, _, car_guard = R.fp_state(g, cand, discs)
            starts[:2] = cand[w.is_state_valid(cand).astype(bool) & ~car_ok & ~car_guard][:2]
        seeds = np.arange(n, dtype=np.uint64) + 900 + 100 * rnd
        planner.set_footprint(None)
        point = plan(planner, starts, goals, seeds)
        planner.set_footprint(fp)
        car = plan(planner, starts, goals, seeds)
        start_ok = R.fp_state(g, starts, discs)[0]
        for q in range(n):
            c = car[q]
            if not start_ok[q]:
                assert c["status"] != 0, q
            if c["status"] == 0:
                successes += 1
                p = c["path"]
                act = np.where(p["kind"][1:] == 2, 1000 + p["prim"][1:], p["prim"][1:])
                v, gd = edges_valid(g, discs, curv, direc, p["poses"][:-1], goals[q], act, p["length"][1:])
                assert v[~gd].all(), (q, np.flatnonzero(~v & ~gd))
            # the whole search tree
            parents, poses, action, length = tree_of(planner, q, c["n_nodes"])
            child = np.flatnonzero(parents >= 0)
            if len(child):
                pp = poses[parents[child]]
                v, gd = edges_valid(g, discs, curv, direc, pp, goals[q], action[child], length[child])
                edges_checked += len(child)
                edges_left_out += int(gd.sum())
                assert v[~gd].all(), (q, child[~v & ~gd][:8])
                short = (action[child] < 1000) & (length[child] < full)
                if short.any():
                    a = action[child][short]
                    fv, fl, fg, _ = R.fp_arcs(g, pp[short], curv[a], full, direc[a], discs)
                    keep = ~fg
                    assert not fv[keep].any()  # a truncated arc: the full one is invalid
                    assert np.abs(length[child][short][keep] - fl[keep].astype(np.float64) * full).max() <= 1e-9
            # did the footprint change this plan?  (the point validator's plan re-marched for the car)
            pt = point[q]
            if pt["status"] == 0 and c["status"] == 0:
                p = pt["path"]
                act = np.where(p["kind"][1:] == 2, 1000 + p["prim"][1:], p["prim"][1:])
                v, gd = edges_valid(g, discs, curv, direc, p["poses"][:-1], goals[q], act, p["length"][1:])
                if not v[~gd].all():
                    changed += 1
        if changed >= 4:
            break
    print("car footprint %d^2: %d rounds, %d plans, %d plans changed by the footprint, %d tree edges re-marched, %d in the guard band" % (n_cells, rnd + 1, successes, changed, edges_checked, edges_left_out))
    assert changed >= 4, (changed, successes)  # a test where the footprint changes no plan shows nothing
    assert edges_checked > 1000 and edges_left_out <= R.MAX_LEFT_OUT * edges_checked, (edges_checked, edges_left_out)


# --------------------------------------------------------------------------------------------------- 10: errors --
def test_footprint_misuse_is_refused_with_a_message():
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError
    w, ms, val, ctx = make_pair(256, 6, 3)
    w2, ms2, val2, _ = make_pair(256, 6, 4, ctx=ctx)
    lib = ms.lib

    def refused(call, *words):
        with pytest.raises(PPError) as e:
            call()
        assert e.value.code == -1, e.value
        assert all(wd in str(e.value) for wd in words), str(e.value)

    refused(lambda: pa.Footprint(ms, []), "1 to 8")
    refused(lambda: pa.Footprint(ms, [(0.1 * i, 0.0, 1.0) for i in range(9)]), "1 to 8")
    refused(lambda: pa.Footprint(ms, [(0.0, 0.0, -1.0)]), "radii")
    refused(lambda: pa.Footprint(ms, [(float("nan"), 0.0, 1.0)]), "finite")
    refused(lambda: pa.Footprint(ms, [(0.0, 0.0, float("inf"))]), "finite")
    fp, foreign = pa.Footprint(ms, R.CAR3), pa.Footprint(ms2, R.CAR3)
    poses = np.zeros((4, 3))
    refused(lambda: val.is_state_valid(poses, footprint=foreign), "another map")
    refused(lambda: val.is_path_valid(poses, 0.1, 1.5, 0, footprint=foreign), "another map")
    refused(lambda: val.is_se2_path_valid(poses, poses + 1.0, footprint=foreign), "another map")
    rows = pa.HybridAStarBatch(val, max_batch=72, max_nodes=16384, search_rows=16)
    assert rows.search_rows > 0
    refused(lambda: rows.set_footprint(fp), "max_batch <= 64", "PP_SEARCH_ROWS=0")
    pipe = pa.HybridAStarPipeline(val, capacity=24, max_nodes=16384, search_rows=16)
    rc = lib.pp_planner_set_footprint(pipe.planner_h, fp.h)
    assert rc == -1 and b"pipeline" in lib.pp_last_error()
    pipe.close()
    single = pa.HybridAStarBatch(val, max_batch=4, max_nodes=32768)
    single.initialize()
    refused(lambda: single.set_footprint(foreign), "another map")
    # clearing the footprint restores the point results
    g = R.Grid(w)
    rng = np.random.RandomState(3)
    starts, goals = R.valid_poses(rng, g, w, 4, R.CAR3), R.valid_poses(rng, g, w, 4, R.CAR3)
    seeds = np.arange(4, dtype=np.uint64)
    base = plan(single, starts, goals, seeds)
    single.set_footprint(fp)
    plan(single, starts, goals, seeds)
    single.set_footprint(None)
    again = plan(single, starts, goals, seeds)
    for b, a in zip(base, again):
        assert (b["status"], b["n_expanded"]) == (a["status"], a["n_expanded"]) and np.array_equal(b["expanded"], a["expanded"])
    assert np.array_equal(val.is_state_valid(starts), w.is_state_valid(starts).astype(bool))


# ----------------------------------------------------------------------------------------------- 11: pyplanning --
def _example_obstacles(nav):
    """the four rectangles of the reference's example script (interfaces/python/scripts/example.py:19-45)"""
    out = []
    for (dx, dy), pose in (((10.0, 1.0), (2.0, 0.0, -math.pi / 4.0)), ((10.0, 1.0), (0.0, 7.5, -math.pi / 4.0)), ((10.0, 1.0), (-8.0, 5.0, math.pi / 2.0)),
                           ((14.0, 1.0), (5.0, -5.0, 0.0))):
        o = nav.Obstacle()
        o.set_shape(nav.RectangleShape(dx, dy))
        o.set_pose(nav.Pose2d(*pose))
        out.append(o)
    return out


def test_footprint_through_pyplanning():
    import importlib
    import os
    import sys
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    space = nav.StateSpaceSE2(nav.Pose2d(-10, -10, -math.pi), nav.Pose2d(10, 10, math.pi))
    m = nav.ObstacleListOccupancyMap(0.1)
    val = nav.StateValidatorOccupancyMap(space, m)
    for o in _example_obstacles(nav):
        assert m.add_obstacle(o)
    nav.GVD(m).update()
    assert nav.rectangle_footprint(4.8, 2.0, 1.0, 3) == R.cover_rectangle(4.8, 2.0, 1.0, 3)
    with pytest.raises(Exception):
        nav.rectangle_footprint(4.8, 2.0, 1.0, 9)
    assert val.footprint == []
    rng = np.random.RandomState(11)
    cand = np.column_stack([rng.uniform(-9.5, 9.5, 4000), rng.uniform(-9.5, 9.5, 4000), rng.uniform(-math.pi, math.pi, 4000)])
    point_ok = np.asarray(val.is_states_valid(cand)).astype(bool)
    val.set_footprint(R.CAR3)
    assert val.footprint == [(ox, oy, float(np.float32(r))) for ox, oy, r in R.CAR3]
    car_ok = np.asarray(val.is_states_valid(cand)).astype(bool)
    assert 0.05 < car_ok.mean() < point_ok.mean()
    assert val.is_state_valid(nav.Pose2d(*cand[car_ok][0])) and not val.is_state_valid(nav.Pose2d(*cand[~car_ok][0]))
    for bad in ([(0.0, 0.0, -1.0)], [(float("nan"), 0.0, 1.0)], [(0.0, 0.0, float("inf"))], [], [(0.1 * i, 0.0, 1.0) for i in range(9)]):
        with pytest.raises(ValueError):
            val.set_footprint(bad)
        # a refused footprint leaves the one that was set
        assert val.footprint == [(ox, oy, float(np.float32(r))) for ox, oy, r in R.CAR3]
        assert np.array_equal(np.asarray(val.is_states_valid(cand)).astype(bool), car_ok)

    # a path type defined by the caller is refused while a footprint is set, and marched on the host again once it is cleared
    class PyLine(nav.PathSE2Base):
        def __init__(self, p, q):
            super().__init__(p, math.hypot(q.x() - p.x(), q.y() - p.y()))
            self.p, self.q = p, q

        def Interpolate(self, r):
            s = nav.Pose2d(0, 0, 0)
            s.position = nav.Point2d((1 - r) * self.p.x() + r * self.q.x(), (1 - r) * self.p.y() + r * self.q.y())
            s.theta = (1 - r) * self.p.theta + r * self.q.theta
            return s

    p, q = nav.Pose2d(*cand[car_ok][0]), nav.Pose2d(*cand[car_ok][1])
    with pytest.raises(RuntimeError) as e:
        val.is_path_valid(PyLine(p, q))
    assert "footprint" in str(e.value)
    # ... and so is a constant-steer arc of a bicycle model whose reference point is not the rear axle, by that name
    off_axle = nav.PathConstantSteer(nav.KinematicBicycleModel(2.6, 0.5), p, 0.2, 3.0, nav.Direction.FORWARD)
    with pytest.raises(RuntimeError) as e:
        val.is_path_valid(off_axle)
    assert "rearToCenter" in str(e.value)
    assert val.is_path_valid(nav.PathConstantSteer(nav.KinematicBicycleModel(2.6, 0.0), p, 0.2, 0.0, nav.Direction.FORWARD))
    ok_fp, last_fp = val.is_path_valid_with_ratio(nav.PathSE2(p, q))
    val.clear_footprint()
    assert val.footprint == []
    assert val.is_path_valid_with_ratio(PyLine(p, q)) == val.is_path_valid_with_ratio(nav.PathSE2(p, q))
    assert np.array_equal(np.asarray(val.is_states_valid(cand)).astype(bool), point_ok)
    val.set_footprint(R.CAR3)
    assert val.is_path_valid_with_ratio(nav.PathSE2(p, q)) == (ok_fp, last_fp)

    # HybridAStar takes the validator's footprint: car-valid starts and goals, first pairs that plan
    poses = cand[car_ok]
    found = 0
    for k in range(0, 40, 2):
        start, goal = poses[k], poses[k + 1]
        algo = nav.HybridAStar(nav.HybridAStarSearchParameters(), 1, 65536)
        assert algo.initialize(val)
        algo.path_interpolation = 0.8
        algo.set_init_state(nav.Pose2d(*start))
        algo.set_goal_state(nav.Pose2d(*goal))
        algo.set_seed(3 + k)
        if algo.search_path() != nav.Status.SUCCESS:
            continue
        found += 1
        nodes = np.array([[n_.x(), n_.y(), n_.theta] for n_ in algo.get_graph_search_nodes()])
        assert np.asarray(val.is_states_valid(nodes)).all(), k  # a node has children only if its own pose is valid; the goal was drawn valid
        for e_ in algo.get_graph_search_path():
            assert val.is_path_valid(e_)
        path = np.array([[s.x(), s.y(), s.theta] for s in algo.get_path()])
        smoothed = np.array([[s.x(), s.y(), s.theta] for s in algo.get_smoothed_path()])
        status = algo.get_stats().smoothing_status
        if len(smoothed):
            all_pass = bool(np.asarray(val.is_states_valid(smoothed)).all())
            if int(status) >= 0:
                assert all_pass and np.array_equal(path, smoothed)
            elif not all_pass:
                assert status == nav.SmoothingStatus.COLLISION and not np.array_equal(path, smoothed) and np.allclose(path[0], start)
        if found >= 3:
            break
    assert found >= 1
