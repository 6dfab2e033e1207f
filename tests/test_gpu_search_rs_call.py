"""-m gpu: the Reeds-Shepp attempt of the rows kernels as a CALLED function (pathplanning_amd/csrc/pp_rows_rs.hpp: rows_rs_attempt).
The call site is divergent -- between one and four rows of a wave enter it -- and everything it hands back (word, t/u/v, checks, validity,
the staged child) feeds counters and pushes that the oracle pins.  Queries whose goal lies 3-8 m from the start have h < 10 from the
first expansion, so EVERY expansion of every row attempts Reeds-Shepp; uniformly drawn queries reach it through the RNG gate, one row at a
time while its neighbours expand.  Batch form (k_hybrid_search_rows<false>), pipeline form (<true>, every slot recycled), the footprint
form (k_hybrid_search_rows_footprint<true>) and the node-capacity exit that now sits behind the call."""
import math

import numpy as np
import pytest

import footprint_ref as R
import oracle_lib as O
from gpu_common import make_pair, valid_random_poses
from test_gpu_footprint import edges_valid
from test_gpu_hybrid import compare, run_pair
from test_gpu_pipeline import check_against_oracle
from test_gpu_pipeline_footprint import assert_is_the_one_wave_search, plan_actions, run_pipe, yardstick

pytestmark = pytest.mark.gpu

N_NEAR = 22  # not a multiple of four: the last wave has idle rows


def near_goal_queries(rng, w, n, valid=None, starts=None):
    """starts anywhere valid, every goal 3-8 m from its start at any bearing and heading (redrawn until valid)"""
    valid = valid or (lambda p: w.is_state_valid(p).astype(bool))
    starts = valid_random_poses(rng, w, n) if starts is None else starts
    goals = np.empty_like(starts)
    for i in range(n):
        while True:
            r, a = rng.uniform(3.0, 8.0), rng.uniform(-math.pi, math.pi)
            g = np.array([starts[i, 0] + r * math.cos(a), starts[i, 1] + r * math.sin(a), rng.uniform(-math.pi, math.pi)])
            if valid(g[None, :])[0]:
                goals[i] = g
                break
    return starts, goals


@pytest.fixture(scope="module")
def world():
    w, ms, val, ctx = make_pair(256, 6, 3)
    # seed 47: on the CPU oracle all 22 solve, all 22 plans end in a Reeds-Shepp edge, 18 queries need more than one attempt (the first three
    # -- the one-wave runs below -- take 5, 9 and 3 attempts), at most 61 expansions a query
    near = near_goal_queries(np.random.RandomState(47), w, N_NEAR) + (np.arange(N_NEAR, dtype=np.uint64) + 500,)
    rng = np.random.RandomState(11)
    rand = (valid_random_poses(rng, w, 24), valid_random_poses(rng, w, 24), np.arange(24, dtype=np.uint64) + 100)  # as test_batch_parity_256
    return dict(w=w, ms=ms, val=val, ctx=ctx, near=near, rand=rand, oracle={})


def oracle_results(world, h, name):
    """the oracle's results of a query set, computed once"""
    if name not in world["oracle"]:
        starts, goals, seeds = world[name]
        world["oracle"][name] = [h.search(starts[q], goals[q], int(seeds[q])) for q in range(len(starts))]
    return world["oracle"][name]


def assert_near_goal_set_exercises_the_call(res):
    assert sum(r["status"] == 0 for r in res) >= 16
    assert sum(r["status"] == 0 and len(r["path_kind"]) > 0 and r["path_kind"][-1] == 2 for r in res) >= 8  # plans that end in a Reeds-Shepp edge
    assert sum(r["n_rs_attempts"] > 1 for r in res) >= 4  # attempts the march rejected


def test_batch_form_near_goal_queries(world, monkeypatch):
    monkeypatch.setenv("PP_SEARCH_ROWS", "1")
    starts, goals, seeds = world["near"]
    planner, res, h = run_pair(world["w"], world["ms"], world["val"], {}, starts, goals, seeds, search_rows=8)
    assert_near_goal_set_exercises_the_call(oracle_results(world, h, "near"))
    assert compare(planner, res, h, starts, goals, seeds) >= 16
    for n in (1, 2, 3):  # a single wave with three, two and one idle rows
        planner, res, h = run_pair(world["w"], world["ms"], world["val"], {}, starts[:n], goals[:n], seeds[:n], search_rows=4)
        assert compare(planner, res, h, starts[:n], goals[:n], seeds[:n]) == sum(r["status"] == 0 for r in oracle_results(world, h, "near")[:n])


def test_batch_form_random_gate_queries(world, monkeypatch):
    monkeypatch.setenv("PP_SEARCH_ROWS", "1")
    starts, goals, seeds = world["rand"]
    planner, res, h = run_pair(world["w"], world["ms"], world["val"], {}, starts, goals, seeds, search_rows=8)
    want = oracle_results(world, h, "rand")
    assert sum(r["n_rng_draws"] for r in want) > 0 and sum(r["n_rs_attempts"] for r in want) > 0
    assert compare(planner, res, h, starts, goals, seeds) >= len(starts) // 2


def test_pipeline_form(world):
    import pathplanning_amd as pa
    pipe = pa.HybridAStarPipeline(world["val"], capacity=16, max_nodes=32768, search_rows=8, log_expansions=True)  # every slot is recycled
    pipe.initialize()
    h = O.Hybrid(world["w"], O.params_array(), table=pipe.nonholo_table())
    for name in ("near", "rand"):
        starts, goals, seeds = world[name]
        solved = []
        run_pipe(pipe, starts, goals, seeds, chunk=7, logged=True,
                 inspect=lambda q, t, r: solved.append(check_against_oracle(pipe, t, r, h, starts[q], goals[q], seeds[q])))
        assert len(solved) == len(starts) and sum(solved) >= (16 if name == "near" else len(starts) // 2)
    pipe.close()


def test_footprint_form_near_goal_queries(world):
    """the near-goal set with the three-disc car through k_hybrid_search_rows_footprint<true>: the one-wave footprint search query by query
    (which tests/test_gpu_footprint.py pins to the numpy restatement), and every edge of every plan re-marched with tests/footprint_ref.py"""
    import pathplanning_amd as pa
    w, ms, val = world["w"], world["ms"], world["val"]
    g = R.Grid(w)
    discs = R.CAR3
    params = pa.HybridAStarSearchParameters()
    _, curv, direc = params.primitives()
    def car_valid(p):  # the restatement's verdict, outside its guard band
        ok, _, _, guard = R.fp_state(g, p, discs)
        return ok & ~guard

    rng = np.random.RandomState(47)
    starts, goals = near_goal_queries(rng, w, N_NEAR, valid=car_valid, starts=R.valid_poses(rng, g, w, N_NEAR, discs))
    seeds = np.arange(N_NEAR, dtype=np.uint64) + 500
    planner = pa.HybridAStarBatch(val, params, max_batch=N_NEAR, max_nodes=32768)
    assert planner.search_rows == 0
    planner.initialize()
    fp = pa.Footprint(ms, discs)
    planner.set_footprint(fp)
    want = yardstick(planner, starts, goals, seeds)
    assert sum(d["n_rs_attempts"] > 0 for d in want) >= 16 and sum(d["status"] == 0 for d in want) >= 8
    pipe = pa.HybridAStarPipeline(val, params, capacity=16, max_nodes=32768, search_rows=8, log_expansions=True)
    pipe.initialize(planner.nonholo_table())
    pipe.set_footprint(fp)
    got, _ = run_pipe(pipe, starts, goals, seeds, chunk=7, logged=True)
    for q in range(N_NEAR):
        assert_is_the_one_wave_search(got[q], want[q], q)
        if got[q]["status"] == 0:
            p = got[q]["path"]
            v, gd = edges_valid(g, discs, curv, direc, p["poses"][:-1], goals[q], plan_actions(p), p["length"][1:])
            assert v[~gd].all(), (q, np.flatnonzero(~v & ~gd))
    pipe.close()
    planner.close()


def test_node_capacity_is_reported_behind_the_call(world, monkeypatch):
    """max_nodes = 64: the query runs out of node records (status -4) in the batch form and in the pipeline form"""
    import pathplanning_amd as pa
    monkeypatch.setenv("PP_SEARCH_ROWS", "1")
    start, goal = [[-11.0, -11.0, 0.0]], [[11.0, 11.0, 0.0]]
    planner = pa.HybridAStarBatch(world["val"], max_batch=1, max_nodes=64, search_rows=4)
    planner.initialize()
    assert planner.search_batch(start, goal, [1])[0].status == -4
    pipe = pa.HybridAStarPipeline(world["val"], capacity=4, max_nodes=64, search_rows=4)
    pipe.initialize(planner.nonholo_table())
    got, _ = run_pipe(pipe, np.array(start), np.array(goal), np.array([1], dtype=np.uint64))
    assert got[0]["status"] == -4
    pipe.close()
    planner.close()
