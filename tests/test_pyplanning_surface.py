"""The pybind11 module keeps the reference's names for the hot-path surface
(interfaces/python/src/pyplanning.cpp:42-122,208-237,320-327,337-357,402-421)."""
import importlib
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nav():
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "pathplanning_amd", "lib"))
    return importlib.import_module("pyplanning")


def test_names_match_reference_bindings(nav):
    # every class / enum the reference module binds (interfaces/python/src/pyplanning.cpp:42-435)
    for name in ("initialize", "Status", "PathPlannerSE2Base", "HybridAStarSearchParameters", "HybridAStarSmootherParameters", "HybridAStarStats", "SmoothingStatus",
                 "HybridAStar", "AStarHeuristicN2", "AStarHeuristicFcnN2", "AStarStatePropagatorN2", "AStarStatePropagatorFcnN2", "PathPlannerN2Base", "AStarN2",
                 "BidirectionalAStarN2", "Point2d", "Pose2d", "GridCellPosition", "Steer", "Direction", "PathSE2Base", "PathSE2", "PathNonHolonomicSE2Base", "PathReedsShepp",
                 "PathConstantSteer", "KinematicBicycleModel", "PathConnectionSE2Base", "PathConnectionSE2", "PathConnectionReedsShepp", "StateSpaceSE2", "OccupancyMap",
                 "ObstacleListOccupancyMap", "Obstacle", "Shape", "CompositeShape", "PolygonShape", "RegularPolygonShape", "RectangleShape", "CircleShape",
                 "StateValidatorSE2Base", "StateValidatorSE2Free", "StateValidatorOccupancyMap", "GVD"):
        assert hasattr(nav, name), name
    for meth in ("initialize", "set_init_state", "set_goal_state", "search_path", "get_path", "get_stats", "get_graph_search_explored_path_set", "get_graph_search_path",
                 "get_graph_search_optimal_cost", "get_smoothed_path", "get_search_parameters", "smoother_parameters", "visualize_obstacle_heuristic", "path_interpolation"):
        assert hasattr(nav.HybridAStar, meth), meth
    for meth in ("initialize_size", "rows", "columns", "set_position", "get_position", "get_occupancy_value", "world_position_to_grid_cell", "is_inside_map"):
        assert hasattr(nav.OccupancyMap, meth), meth
    assert nav.Status.SUCCESS != nav.Status.FAILURE
    p = nav.HybridAStarSearchParameters(2.0, 0.0, 1.0, 1.0, 1.0, 5, 1.0, 0.0872)  # pyplanning.cpp:75 (8-argument constructor)
    assert p.wheelbase == 2.6 and p.num_generated_motion == 5 and p.angular_resolution == 0.0872


def test_every_name_the_reference_module_binds_is_bound(nav):
    """tests/golden/pyplanning_bound_names.json = the class, enum, method, property and value NAMES extracted from the reference's
    interfaces/python/src/pyplanning.cpp by tests/golden/make_pyplanning_names.py (118 members of 42 classes): none may be missing
    here -- including the typo'd "is_occupied)" (pyplanning.cpp:351), which a caller of the reference can only reach by getattr."""
    import json
    import os
    names = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyplanning_bound_names.json")))
    assert len(names["classes"]) >= 42
    missing = [n for n in names["module"] if not hasattr(nav, n)]
    for cls, info in names["classes"].items():
        if not hasattr(nav, cls):
            missing.append(cls)
            continue
        missing += ["%s.%s" % (cls, m) for m in info["members"] if not hasattr(getattr(nav, cls), m)]
    assert missing == []
    m = nav.OccupancyMap(0.5)
    m.initialize_size(8.0, 8.0)
    assert getattr(m, "is_occupied)")(nav.GridCellPosition(1, 1)) == m.is_occupied(nav.GridCellPosition(1, 1))
    with pytest.raises(TypeError):  # as in the reference: the return type is not a bound class
        m.get_obstacle_map()


def test_state_space_samplers_follow_the_reference_random(nav):
    """StateSpaceSE2::SampleUniform / SampleGaussian (state_space_se2.cpp:27-52, pyplanning.cpp:325-326) on the global mt19937_64 of
    utils/random.h: with the same seed, the stream of the reference's own random.h (compiled into oracle/_ref, or its recorded output:
    tests/ref_vectors.py)."""
    import ref_vectors as R
    lb, ub, mean, std, n = R.SE2_LB, R.SE2_UB, R.SE2_MEAN, R.SE2_STD, R.SE2_DRAWS
    uni, gau = R.reference().rng_se2(R.SE2_SEED, n, lb, ub, mean, std)
    ss = nav.StateSpaceSE2(nav.Pose2d(*lb), nav.Pose2d(*ub))
    nav.seed_random(R.SE2_SEED)
    got_u = np.array([[p.x(), p.y(), p.theta] for p in (ss.sample_uniform() for _ in range(n))])
    got_g = np.array([[p.x(), p.y(), p.theta] for p in (ss.sample_gaussian(nav.Pose2d(*mean), nav.Pose2d(*std)) for _ in range(n))])
    assert np.array_equal(got_u, uni)
    assert np.array_equal(got_g, np.clip(gau, lb, ub))  # EnforceBounds (std::clamp per component)
    assert (np.clip(gau, lb, ub) != gau).any()  # the clamp is exercised
    assert all(ss.validate_bounds(nav.Pose2d(*r)) for r in got_u[:20])


def test_host_side_value_types(nav):
    a = nav.Pose2d(1.0, 2.0, 7.0)  # constructor wraps theta (geometry/2dplane.h:19-22)
    assert abs(a.theta - (7.0 - 2 * np.pi)) < 1e-15
    assert (nav.Point2d(1, 2) + nav.Point2d(3, 4)) == nav.Point2d(4, 6)
    ss = nav.StateSpaceSE2(nav.Pose2d(-10, -10, -np.pi), nav.Pose2d(10, 10, np.pi))
    assert ss.validate_bounds(nav.Pose2d(0, 0, 0)) and not ss.validate_bounds(nav.Pose2d(11, 0, 0))
    m = nav.OccupancyMap(0.1)
    m.initialize_size(20.0, 20.0)
    assert (m.rows(), m.columns()) == (200, 200)
    c = m.world_position_to_grid_cell(nav.Point2d(0.05, -9.95), True)
    assert (c.row, c.col) == (100, 0)
    assert m.world_position_to_grid_cell(nav.Point2d(11.0, 0.0), True).row == -1


@pytest.mark.gpu
def test_reference_python_flow_on_gpu(nav):
    """The flow of interfaces/python/tests/test_pypath_planning.py:60-99 (map -> validator -> HybridAStar), grids set from the oracle world."""
    import oracle_lib as O
    w = O.synthetic_world(256, 6, 3)
    lb, ub = w.lb, w.ub
    ss = nav.StateSpaceSE2(nav.Pose2d(lb[0], lb[1], lb[2]), nav.Pose2d(ub[0], ub[1], ub[2]))
    m = nav.OccupancyMap(0.1)
    val = nav.StateValidatorOccupancyMap(ss, m)
    assert (m.rows(), m.columns()) == (w.rows, w.cols)
    m.set_grids(w.occ(), w.d2(), w.pathcost())
    rng = np.random.RandomState(0)
    poses = np.column_stack([rng.uniform(-13, 13, 2000), rng.uniform(-13, 13, 2000), rng.uniform(-3, 3, 2000)])
    assert np.array_equal(val.is_states_valid(poses).astype(bool), w.is_state_valid(poses).astype(bool))
    assert val.is_state_valid(nav.Pose2d(*poses[0])) == bool(w.is_state_valid(poses[:1])[0])
    algo = nav.HybridAStar(nav.HybridAStarSearchParameters(), 4)
    assert algo.initialize(val)
    algo.set_init_state(nav.Pose2d(-10.0, -10.0, 0.0))
    algo.set_goal_state(nav.Pose2d(10.0, 10.0, 0.0))
    algo.set_seed(7)
    assert algo.search_path() == nav.Status.SUCCESS
    path = algo.get_path()
    h = O.Hybrid(w)
    r = h.search([-10.0, -10.0, 0.0], [10.0, 10.0, 0.0], 7)
    assert len(path) == len(r["path_poses"])
    got = np.array([[p.x(), p.y(), p.theta] for p in path])
    assert np.abs(got - r["path_poses"]).max() < 1e-5
    assert abs(algo.get_graph_search_optimal_cost() - r["cost"]) < 1e-5
    res = algo.search_batch(np.array([[-10.0, -10.0, 0.0], [9.0, -9.0, 1.0]]), np.array([[10.0, 10.0, 0.0], [-9.0, 8.0, -2.0]]), np.array([7, 8], dtype=np.uint64))
    assert res[0][0] == 0 and abs(res[0][1] - r["cost"]) < 1e-5


@pytest.mark.gpu
def test_cpp_plugin_mirror_of_reference_tests():
    import subprocess
    from pathplanning_amd import build
    exe = build.build_plugin_test(verbose=False)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plugin tests ok" in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("queues", [None, "2"])
def test_pipeline_states_its_hardware_queue_precondition(queues):
    """A C++ host with whatever hardware queues its environment gives the HIP runtime (None; tests/conftest.py caps them at 2), or with 2:
    pp_pipeline_create either finds that its streams do run side by side and the pipeline works, or returns an error that names
    GPU_MAX_HW_QUEUES -- it does not run ten times slower in silence (include/pp_hip.h).  (More than 2 queues is not tried: the GPU may be
    shared with other processes.)"""
    import os
    import subprocess
    from pathplanning_amd import build
    exe = build.build_plugin_test(verbose=False)
    env = dict(os.environ)
    env.pop("PP_PIPE_ALLOW_SHARED_QUEUES", None)
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = queues
    out = subprocess.run([exe, "--queues"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    ran = "pipeline accepted and ran" in out.stdout
    refused = "pipeline refused" in out.stdout and "GPU_MAX_HW_QUEUES" in out.stdout
    assert ran != refused, out.stdout
    if queues == "2":
        assert refused, out.stdout


def test_path_value_types_on_the_host(nav):
    """PathSE2 / PathConstantSteer / KinematicBicycleModel / Pose2d composition are plain host arithmetic in the mirror
    (paths/path_se2.cpp, path_constant_steer.cpp, models/kinematic_bicycle_model.cpp, geometry/2dplane.h:47-79)."""
    import oracle_lib as O
    for name in ("Steer", "PathSE2Base", "PathSE2", "PathNonHolonomicSE2Base", "PathReedsShepp", "PathConstantSteer", "KinematicBicycleModel", "PathConnectionSE2Base",
                 "PathConnectionSE2", "PathConnectionReedsShepp", "StateValidatorSE2Free", "AStarN2", "BidirectionalAStarN2", "AStarHeuristicFcnN2", "AStarStatePropagatorFcnN2",
                 "PathPlannerN2Base"):
        assert hasattr(nav, name), name
    for meth in ("get_initial_state", "get_final_state", "interpolate", "truncate", "get_length"):
        assert hasattr(nav.PathSE2Base, meth), meth
    assert hasattr(nav.StateValidatorSE2Base, "is_path_valid") and hasattr(nav.HybridAStar, "get_graph_search_path")
    a, b = nav.Pose2d(1.0, 2.0, 0.5), nav.Pose2d(4.0, 6.0, -1.0)
    p = nav.PathSE2(a, b)
    assert p.get_length() == 5.0
    mid = p.interpolate(0.25)
    assert (mid.x(), mid.y(), mid.theta) == (0.75 * 1.0 + 0.25 * 4.0, 0.75 * 2.0 + 0.25 * 6.0, 0.75 * 0.5 + 0.25 * -1.0)
    p.truncate(0.5)
    assert p.get_length() == 2.5 and p.get_final_state().x() == 2.5
    # a + (b - a) == b
    c = a + (b - a)
    assert abs(c.x() - b.x()) < 1e-12 and abs(c.y() - b.y()) < 1e-12 and abs(c.theta - b.theta) < 1e-12
    model = nav.KinematicBicycleModel(2.6, 0.0)
    rng = np.random.RandomState(1)
    frm = np.column_stack([rng.uniform(-5, 5, 200), rng.uniform(-5, 5, 200), rng.uniform(-3, 3, 200)])
    steer = rng.uniform(-0.9, 0.9, 200)
    steer[:5] = 0.0
    dist = rng.uniform(0, 3, 200)
    direc = rng.randint(0, 2, 200)
    want = O.constant_steer(frm, steer, dist, direc)
    for i in range(200):
        arc = nav.PathConstantSteer(model, nav.Pose2d(*frm[i]), steer[i], dist[i], nav.Direction.BACKWARD if direc[i] else nav.Direction.FORWARD)
        f = arc.get_final_state()
        assert (f.x(), f.y(), f.theta) == tuple(want[i])  # same closed form, same libm: identical
        assert arc.get_direction(0.3) == (nav.Direction.BACKWARD if direc[i] else nav.Direction.FORWARD)
    ss = nav.StateSpaceSE2(nav.Pose2d(-10, -10, -np.pi), nav.Pose2d(10, 10, np.pi))
    free = nav.StateValidatorSE2Free(ss)
    assert free.is_state_valid(nav.Pose2d(0, 0, 0)) and not free.is_state_valid(nav.Pose2d(11, 0, 0))
    assert free.is_path_valid(nav.PathSE2(a, nav.Pose2d(50, 50, 0)))  # state_validator_free.h:24-29: every path is valid


@pytest.mark.gpu
def test_generic_is_path_valid_and_graph_search_path_on_gpu(nav):
    """StateValidator::IsPathValid(const Path&, float*) over every path type of the reference (validated on the GPU) and over
    a path type defined in Python (sampled through its own interpolate, marched on the host copy of the distance grid);
    PathConnectionReedsShepp / PathReedsShepp through the module; HybridAStar.get_graph_search_path()."""
    import oracle_lib as O
    from gpu_common import valid_random_poses
    w = O.synthetic_world(256, 6, 3)
    lb, ub = w.lb, w.ub
    ss = nav.StateSpaceSE2(nav.Pose2d(lb[0], lb[1], lb[2]), nav.Pose2d(ub[0], ub[1], ub[2]))
    m = nav.OccupancyMap(0.1)
    val = nav.StateValidatorOccupancyMap(ss, m)
    res = np.float64(np.float32(0.1))
    m.set_grids(w.occ(), w.d2(), w.pathcost())
    rng = np.random.RandomState(4)
    a, b = valid_random_poses(rng, w, 120), valid_random_poses(rng, w, 120)
    b[:60, :2] = a[:60, :2] + rng.uniform(-4, 4, (60, 2))
    # Reeds-Shepp
    conn = nav.PathConnectionReedsShepp(2.0, 0.0, 1.0, 1.0)
    P = O.rs_connect(a, b, 2.0)
    wv, wl = O.rs_paths_valid(w, P)
    n_valid = 0
    for i in range(len(a)):
        path = conn.connect(nav.Pose2d(*a[i]), nav.Pose2d(*b[i]))
        assert isinstance(path, nav.PathReedsShepp)
        if path.word != P["word"][i]:
            continue  # libm near-tie between two words (see test_gpu_paths.py)
        assert abs(path.get_length() - P["length"][i]) < 1e-9
        ok, last = val.is_path_valid_with_ratio(path)
        assert ok == wv[i] and last == wl[i]
        n_valid += ok
        f = path.get_final_state()
        assert abs(f.x() - P["final_pose"][i][0]) < 1e-9 and abs(f.theta - P["final_pose"][i][2]) < 1e-9
        mid = path.interpolate(0.37)
        wp, wd = O.rs_path_interpolate(P[i:i + 1], 0.37)
        assert abs(mid.x() - wp[0][0]) < 1e-9 and int(path.get_direction(0.37)) == wd[0]
        assert len(path.get_cusp_point_ratios()) == len(O.rs_path_cusps(P[i:i + 1])[0])
    assert 5 < n_valid < 115
    # PathSE2 on the GPU, and the same line as a Python-defined path type: the host march must agree with the kernel
    sv, sl = O.se2_paths_valid(w, a, b)

    class PyLine(nav.PathSE2Base):
        def __init__(self, p, q):
            super().__init__(p, math.hypot(q.x() - p.x(), q.y() - p.y()))
            self.p, self.q = p, q

        def Interpolate(self, r):
            s = nav.Pose2d(0, 0, 0)
            s.position = nav.Point2d((1 - r) * self.p.x() + r * self.q.x(), (1 - r) * self.p.y() + r * self.q.y())
            s.theta = (1 - r) * self.p.theta + r * self.q.theta
            return s

    for i in range(len(a)):
        p, q = nav.Pose2d(*a[i]), nav.Pose2d(*b[i])
        ok, last = val.is_path_valid_with_ratio(nav.PathSE2(p, q))
        assert ok == sv[i] and last == sl[i]
        line = PyLine(p, q)
        ok2, last2 = val.is_path_valid_with_ratio(line)
        assert ok2 == sv[i] and last2 == sl[i]
    # constant-steer arcs
    model = nav.KinematicBicycleModel(2.6, 0.0)
    steer = rng.uniform(-0.9, 0.9, len(a))
    cv, cl = w.is_path_valid_csteer(a, steer, 3.0, 0)
    for i in range(len(a)):
        ok, last = val.is_path_valid_with_ratio(nav.PathConstantSteer(model, nav.Pose2d(*a[i]), steer[i], 3.0, nav.Direction.FORWARD))
        assert ok == bool(cv[i]) and last == cl[i]
    # the solution as path objects: edges chain up, lengths add up to the search's path, last edge is the RS connection
    algo = nav.HybridAStar(nav.HybridAStarSearchParameters(), 4)
    assert algo.initialize(val)
    algo.set_init_state(nav.Pose2d(-10.0, -10.0, 0.0))
    algo.set_goal_state(nav.Pose2d(10.0, 10.0, 0.0))
    algo.set_seed(7)
    assert algo.search_path() == nav.Status.SUCCESS
    nodes = algo.get_path()
    edges = algo.get_graph_search_path()
    assert len(edges) == len(nodes) - 1
    r = O.Hybrid(w).search([-10.0, -10.0, 0.0], [10.0, 10.0, 0.0], 7)
    for k, e in enumerate(edges):
        s0, s1 = e.get_initial_state(), e.get_final_state()
        assert abs(s0.x() - nodes[k].x()) < 1e-12 and abs(s1.x() - nodes[k + 1].x()) < 1e-6 and abs(s1.y() - nodes[k + 1].y()) < 1e-6
        assert abs(e.get_length() - r["path_length"][k + 1]) < 1e-6
        assert val.is_path_valid(e)
    assert isinstance(edges[-1], nav.PathReedsShepp) and isinstance(edges[0], nav.PathConstantSteer)


def _example_obstacles(nav, scale=1.0):
    """The four rectangles of interfaces/python/scripts/example.py:19-45 (poses as there)."""
    out = []
    for (dx, dy), pose in (((10.0, 1.0), (2.0, 0.0, -math.pi / 4.0)), ((10.0, 1.0), (0.0, 7.5, -math.pi / 4.0)), ((10.0, 1.0), (-8.0, 5.0, math.pi / 2.0)),
                           ((14.0, 1.0), (5.0, -5.0, 0.0))):
        o = nav.Obstacle()
        o.set_shape(nav.RectangleShape(dx, dy))
        o.set_pose(nav.Pose2d(*pose))
        out.append((o, dx, dy, pose))
    return out


@pytest.mark.gpu
def test_reference_example_script_flow_headless(nav, tmp_path):
    """interfaces/python/scripts/example.py without the plotting: ObstacleListOccupancyMap + shapes + GVD + HybridAStar, every
    grid built on the device.  Occupancy must equal the oracle's rasterisation; the search must equal the oracle's search on
    the same (device-built) fields."""
    import oracle_lib as O
    state_space = nav.StateSpaceSE2(nav.Pose2d(-10, -10, -math.pi), nav.Pose2d(10, 10, math.pi))
    m = nav.ObstacleListOccupancyMap(0.1)
    validator = nav.StateValidatorOccupancyMap(state_space, m)
    w = O.World(10.0, 10.0, 0.1)
    positions = []
    for o, dx, dy, pose in _example_obstacles(nav):
        assert m.add_obstacle(o) and not m.add_obstacle(o)
        w.add_rectangle(dx, dy, pose)
        positions.append(o.get_boundary_world_position())
        cells = o.get_boundary_grid_cell_position(m)
        assert len(cells) > 100 and all(m.is_occupied(c) for c in cells[:5])
    assert m.get_num_obstacles() == 4 and len(positions[0]) == 4
    assert np.array_equal(m.occupancy(), w.occ())
    gvd = nav.GVD(m)
    gvd.update()
    ppm = tmp_path / "test.ppm"
    gvd.visualize(str(ppm))
    assert ppm.stat().st_size > 200 * 200 * 3
    w.update()
    d = np.array([[gvd.get_distance_to_nearest_obstacle(r, c) for c in range(0, 200, 7)] for r in range(0, 200, 7)])
    ref = (np.sqrt(w.d2()[::7, ::7].astype(np.float64)) * np.float64(np.float32(0.1))).astype(np.float32)
    assert (d == ref).mean() > 0.995 and np.abs(d - ref).max() < 0.02
    assert gvd.get_path_cost(100, 100) >= 0.0 and gvd.get_distance_to_nearest_voronoi_edge(nav.GridCellPosition(100, 100)) >= 0.0
    algo = nav.HybridAStar()
    algo.set_init_state(nav.Pose2d(0.0, -9.0, 0.0))
    algo.set_goal_state(nav.Pose2d(8.0, 8.0, 0.0))
    assert algo.initialize(validator)
    algo.path_interpolation = 0.8
    algo.set_seed(3)
    assert algo.search_path() == nav.Status.SUCCESS
    nodes = algo.get_graph_search_nodes()
    edges = algo.get_graph_search_path()
    assert len(edges) == len(nodes) - 1 and abs(nodes[-1].x() - 8.0) < 1e-6
    ratios = list(np.linspace(0.0, 1.0, 10))
    for e in edges:
        assert len(e.interpolate(ratios)) == 10
    # every edge of the search tree (example.py:69-81 plots them) and the obstacle heuristic image
    explored = algo.get_graph_search_explored_path_set()
    assert len(explored) >= len(edges) and all(len(e.interpolate(ratios)) == 10 for e in explored[:20])
    tree_ends = {(round(e.get_final_state().x(), 9), round(e.get_final_state().y(), 9)) for e in explored}
    assert all((round(n_.x(), 9), round(n_.y(), 9)) in tree_ends for n_ in nodes[1:])
    img = tmp_path / "heur.ppm"
    algo.visualize_obstacle_heuristic(str(img))
    assert img.stat().st_size > 200 * 200 * 3
    # GetPath(): the composite path sampled every 0.8 m, smoothed when the smoother succeeds (hybrid_a_star.cpp:260-303)
    path = algo.get_path()
    stats = algo.get_stats()
    assert stats.graph_search_status == nav.Status.SUCCESS
    assert len(path) > len(nodes) or algo.path_interpolation > 1.4
    # (the last sample is the goal only when the path length falls within half a step of a multiple of the step, hybrid_a_star.cpp:276-287)
    assert abs(path[0].x() - 0.0) < 1e-9 and abs(path[0].y() + 9.0) < 1e-9 and math.hypot(path[-1].x() - 8.0, path[-1].y() - 8.0) < 0.8 + 1e-9
    assert len(algo.get_smoothed_path()) == len(path)
    assert algo.smoother_parameters.max_curvature == np.float32(0.5) and algo.smoother_parameters.max_iterations == 2000
    # the oracle on the device-built fields
    d2 = np.rint((np.array([[m.get_distance_to_nearest_obstacle(r, c) for c in range(200)] for r in range(200)], dtype=np.float64) / np.float64(np.float32(0.1))) ** 2)
    w.set_d2(d2.astype(np.int32))
    w.set_pathcost(np.array([[gvd.get_path_cost(r, c) for c in range(200)] for r in range(200)], dtype=np.float32))
    r = O.Hybrid(w).search([0.0, -9.0, 0.0], [8.0, 8.0, 0.0], 3)
    assert r["status"] == 0 and len(r["path_poses"]) == len(nodes)
    assert np.abs(np.array([[p.x(), p.y(), p.theta] for p in nodes]) - r["path_poses"]).max() < 1e-5
    assert abs(algo.get_graph_search_optimal_cost() - r["cost"]) < 1e-5
    # ... and the oracle's post-processing on the device's label grids
    no = np.array([[[c.row, c.col] for c in (gvd.get_nearest_obstacle_cell(r_, c_) for c_ in range(200))] for r_ in range(200)], dtype=np.int32)
    ne = np.array([[[c.row, c.col] for c in (gvd.get_nearest_voronoi_edge_cell(r_, c_) for c_ in range(200))] for r_ in range(200)], dtype=np.int32)
    want = O.postprocess(w, r, [8.0, 8.0, 0.0], path_interpolation=0.8, nearest=(no, ne))
    assert want["n_points"] == len(path) and int(stats.smoothing_status) == want["status"]
    got = np.array([[p.x(), p.y(), p.theta] for p in path])
    assert np.abs(got - (want["smoothed"] if want["status"] >= 0 else want["resampled"])).max() < 1e-5
    # removing an obstacle frees its outline again; the fields are rebuilt at the next search
    o0 = _example_obstacles(nav)[0][0]
    assert not m.remove_obstacle(o0)  # a different object, not on the map


@pytest.mark.gpu
def test_reference_grid_example_script_flow_headless(nav):
    """interfaces/python/scripts/example_a_star_grid.py without the plotting: obstacle outlines rasterised on the device, grid
    A* and bidirectional A* on the host with Python callbacks."""
    import oracle_lib as O
    m = nav.ObstacleListOccupancyMap(0.5)
    m.initialize_size(20, 20)
    w = O.World(10.0, 10.0, 0.5)
    for (dx, dy), pose in (((10.0, 1.0), (2.0, 0.0, -math.pi / 4.0)), ((10.0, 1.0), (0.0, 7.0, -math.pi / 4.0)), ((10.0, 1.0), (-8.0, 5.0, math.pi / 2.0)),
                           ((14.0, 1.0), (5.0, -5.0, 0.0))):
        o = nav.Obstacle()
        o.set_shape(nav.RectangleShape(dx, dy))
        o.set_pose(nav.Pose2d(*pose))
        m.add_obstacle(o)
        w.add_rectangle(dx, dy, pose)
    assert (m.rows(), m.columns()) == (40, 40) and np.array_equal(m.occupancy(), w.occ())

    def cost(a, b):
        return math.sqrt((a.row - b.row) ** 2 + (a.col - b.col) ** 2)

    prop, heur = nav.AStarStatePropagatorFcnN2(m, cost), nav.AStarHeuristicFcnN2(cost)
    uni = nav.AStarN2()
    uni.set_init_state(nav.GridCellPosition(1, 1))
    uni.set_goal_state(nav.GridCellPosition(35, 35))
    uni.initialize(prop, heur)
    assert uni.search_path() == nav.Status.SUCCESS
    want = O.grid_astar(w, (1, 1), (35, 35))
    assert [(c.row, c.col) for c in uni.get_path()] == [tuple(c) for c in want["path"]] and uni.get_optimal_cost() == want["cost"]
    hf, hr = nav.BidirectionalAStarN2.get_average_heuristic_pair(heur, heur)
    bi = nav.BidirectionalAStarN2()
    bi.set_init_state(nav.GridCellPosition(1, 1))
    bi.set_goal_state(nav.GridCellPosition(35, 35))
    bi.initialize(prop, prop, hf, hr)
    assert bi.search_path() == nav.Status.SUCCESS
    wb = O.grid_astar(w, (1, 1), (35, 35), bidirectional=True, inner_goal_f=(35, 35), inner_goal_r=(35, 35))
    assert [(c.row, c.col) for c in bi.get_path()] == [tuple(c) for c in wb["path"]]
    assert abs(bi.get_optimal_cost() - uni.get_optimal_cost()) < 1e-9
    # the same two searches as a batch on the device (pyplanning.GridAStarBatch; Euclidean cost / heuristic): identical to the host engine
    batch = nav.GridAStarBatch(m)
    inits = [nav.GridCellPosition(1, 1), nav.GridCellPosition(35, 35), nav.GridCellPosition(3, 30)]
    goals = [nav.GridCellPosition(35, 35), nav.GridCellPosition(1, 1), nav.GridCellPosition(30, 3)]
    res = batch.search_batch(inits, goals, want_expanded=True)
    assert res[0].status == nav.Status.SUCCESS and res[0].cost == uni.get_optimal_cost()
    assert [(c.row, c.col) for c in res[0].path] == [(c.row, c.col) for c in uni.get_path()]
    assert [(c.row, c.col) for c in res[0].expanded] == [(c.row, c.col) for c in uni.get_expansion_order()]
    for q in range(3):
        want_q = O.grid_astar(w, (inits[q].row, inits[q].col), (goals[q].row, goals[q].col))
        assert [(c.row, c.col) for c in res[q].path] == [tuple(c) for c in want_q["path"]] and res[q].cost == want_q["cost"]
    resb = batch.search_batch(inits, goals, bidirectional=True, want_expanded=True)
    for q in range(3):
        want_q = O.grid_astar(w, (inits[q].row, inits[q].col), (goals[q].row, goals[q].col), bidirectional=True,
                              inner_goal_f=(goals[q].row, goals[q].col), inner_goal_r=(inits[q].row, inits[q].col))
        assert [(c.row, c.col) for c in resb[q].path] == [tuple(c) for c in want_q["path"]] and resb[q].cost == want_q["cost"]
        assert [(c.row, c.col) for c in resb[q].expanded_reverse] == [tuple(c) for c in want_q["explored_reverse"]]
