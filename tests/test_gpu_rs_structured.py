"""-m gpu: Reeds-Shepp on structured poses (tests/rs_structured.py; preconditions in tests/test_rs_structured_host.py).  Every other
Reeds-Shepp test draws its pose pairs at random and forgives word mismatches as libm noise; here the pairs are what a planner is fed --
round offsets, headings on multiples of pi / 4 -- with exact cost ties, motions of length 0 and cusps at ratio 0 and 1, and nothing is
forgiven: outside the pairs that the oracle itself flags as fragile (a one-ulp nudge of an input flips its word) the device must return the
oracle's word; on the flagged pairs it may differ, but only into a word of the probed set whose record, integrated independently, reaches
the goal.
  a. pp_rs_solve / pp_rs_connect (the sequential argmin of rs::optimal_word), three cost settings;
  b. interpolate / truncate / cusp ratios on identical records at the junction ratios and their float neighbours;
  c. the validity marches (point validator: equal to the oracle; footprint: the numpy restatement);
  d. the three argmin forms inside a search: one-wave kernel, rows kernel, pipeline, footprint rows kernel, on structured queries that the
     oracle reproduces under every one-ulp nudge."""
import numpy as np
import pytest

import footprint_ref as R
import oracle_lib as O
import rs_structured as S
from gpu_common import make_pair
from test_gpu_footprint import assert_equal_outside_guard, edges_valid
from test_gpu_hybrid import compare, run_pair
from test_gpu_paths import same_records
from test_gpu_pipeline import check_against_oracle
from test_gpu_pipeline_footprint import assert_is_the_one_wave_search, plan_actions, run_pipe, yardstick

pytestmark = pytest.mark.gpu

RMIN = 2.0


@pytest.fixture(scope="module")
def pairs():
    return S.structured_pairs(RMIN)


# ------------------------------------------------------------------------------------------- a: solver and connect --
@pytest.mark.parametrize("costs", S.COSTS)
def test_solver_and_connect_on_structured_pairs(pairs, costs):
    import pathplanning_amd as pa
    ctx = pa.Context(0)
    a, b = pairs
    rev, fwd, sw = costs
    mask, seen = S.flagged(a, b, RMIN, costs)
    assert 0 < mask.mean() < 0.03
    keep = ~mask
    rows = np.arange(len(a))
    wo, tuvo, costo, sego = O.rs_optimal_batch(a, b, RMIN, rev, fwd, sw)
    want = O.rs_connect(a, b, RMIN, rev, fwd, sw)
    word, tuv, cost, seg = pa.ReedsSheppSolver(ctx).get_optimal_path(a, b, RMIN, rev, fwd, sw)
    got = pa.ReedsSheppPaths(ctx, RMIN, sw, rev, fwd).connect(a, b)
    zero, tiny = S.zero_or_tiny(got)
    must = mask | zero | tiny | S.zero_or_tiny(want)[0] | S.zero_or_tiny(want)[1]
    e_dev = S.pose_error(S.integrate_records(got, must), b)
    e_ora = S.pose_error(S.integrate_records(want, must), b)
    diff_solve, diff_connect = word != wo, got["word"] != want["word"]
    print("costs %s: flagged share %.4f (%d of %d); unflagged mismatches solve %d connect %d; flagged and different solve %d connect %d; "
          "integrate-vs-goal on the flagged pairs: oracle max %.3g device max %.3g; on all pairs: oracle %.3g device %.3g"
          % (costs, mask.mean(), mask.sum(), len(a), (diff_solve & keep).sum(), (diff_connect & keep).sum(), (diff_solve & mask).sum(),
             (diff_connect & mask).sum(), e_ora[mask].max(), e_dev[mask].max(), e_ora.max(), e_dev.max()))
    for q in np.flatnonzero((diff_solve | diff_connect) & keep)[:8]:
        print("  unflagged mismatch at pair %d: %s -> %s, oracle word %d cost %r, solve word %d cost %r, connect word %d"
              % (q, a[q].tolist(), b[q].tolist(), wo[q], costo[q], word[q], cost[q], got["word"][q]))
    # unflagged: no fractions
    assert np.array_equal(word[keep], wo[keep])
    assert np.abs(tuv[keep] - tuvo[keep]).max() < 1e-9
    assert np.abs(seg[keep] - sego[keep]).max() < 1e-9
    assert np.allclose(cost[keep], costo[keep], rtol=2e-7, atol=0)
    assert np.array_equal(got["word"][keep], want["word"][keep])
    assert (np.abs(got["final_pose"][:, 2]) <= np.pi).all()
    print("  end headings 2 pi apart (+pi on one side, -pi on the other): %d" % (np.abs(got["final_pose"][:, 2] - want["final_pose"][:, 2]) > 6.0)[keep].sum())
    same_records(S.folded(got[keep]), S.folded(want[keep]))
    assert np.allclose(got["cost"][keep], want["cost"][keep], rtol=2e-7, atol=0)
    # flagged: only into a legitimate answer
    for q in np.flatnonzero(mask & (~seen[rows, word] | ~seen[rows, got["word"]]))[:12]:
        print("  flagged pair %d outside its probed set %s: %s -> %s, oracle word %d cost %r, solve word %d cost %r, connect word %d"
              % (q, np.flatnonzero(seen[q]).tolist(), a[q].tolist(), b[q].tolist(), wo[q], costo[q], word[q], cost[q], got["word"][q]))
    assert seen[rows[mask], word[mask]].all() and seen[rows[mask], got["word"][mask]].all()
    used = (got["direction"] != S.NO_MOTION) & np.isfinite(got["motion_length"])
    assert np.array_equal(got["length"], S.record_length(got, used))
    assert e_dev[mask].max() <= max(8 * e_ora[mask].max(), 1e-13), (e_dev[mask].max(), e_ora[mask].max())


# --------------------------------------------------------------------------- b: path operations on identical records --
@pytest.mark.parametrize("costs", S.COSTS[:2])
def test_path_operations_at_the_junction_ratios(pairs, costs):
    import pathplanning_amd as pa
    ctx = pa.Context(0)
    a, b = pairs
    rev, fwd, sw = costs
    rs = pa.ReedsSheppPaths(ctx, RMIN, sw, rev, fwd)
    P = O.rs_connect(a, b, RMIN, rev, fwd, sw)  # identical inputs for both sides
    J = S.junction_ratios(P)
    zero, tiny = S.zero_or_tiny(P)
    assert zero.sum() > 100 and tiny.sum() > 100 and (P["length"] == 0.0).sum() >= 20
    assert ((J[:, :15] == 1.0).any(axis=1) & (P["length"] > 0)).sum() > 1000 and ((J[:, :15] == 0.0).any(axis=1)).sum() > 100

    def same_cusps(recs):
        g, w = rs.get_cusp_point_ratios(recs), O.rs_path_cusps(recs)
        assert [len(x) for x in g] == [len(x) for x in w]
        assert all(np.abs(x - y).max() < 1e-12 for x, y in zip(g, w) if len(x))
        return w

    cusps = same_cusps(P)
    assert sum(1 for c in cusps if len(c) and ((c == 0.0).any() or (c >= 1.0).any())) >= 30
    for col in range(J.shape[1]):
        ratio = J[:, col]
        gp, gd = rs.interpolate(P, ratio)
        wp, wd = O.rs_path_interpolate(P, ratio)
        assert np.array_equal(gd, wd), (col, int((gd != wd).sum()), np.flatnonzero(gd != wd)[:5])
        assert np.abs(gp - wp).max() < 1e-9, col
        T = O.rs_path_truncate(P, ratio)
        cut = rs.truncate(P, ratio)
        same_records(cut, T)
        fixed = rs.truncate(P, ratio, q11=False)  # the intended behaviour has no oracle: against the Q11 form where they must agree, and itself
        assert np.array_equal(fixed["final_pose"], cut["final_pose"]) and np.array_equal(fixed["length"], cut["length"])
        fp, _ = rs.interpolate(fixed, 1.0)
        ok = (ratio >= 0.0) & (ratio <= 1.0)
        assert np.abs(S.folded_poses(fp[ok]) - S.folded_poses(fixed["final_pose"][ok])).max() < 1e-9, col
        if col % 3 == 0 or col >= 15:
            same_records(rs.truncate(T, 0.5), O.rs_path_truncate(T, 0.5))  # truncated once more: mid-way, and at its own first junction
            JT = S.junction_ratios(T)[:, 0]
            same_records(rs.truncate(T, JT), O.rs_path_truncate(T, JT))
            same_cusps(T)


# ---------------------------------------------------------------------------------------------- c: validity marches --
def test_validity_marches_over_structured_paths():
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    a, b = S.structured_pairs(1.0)
    # off the cell boundaries (the restatement's guard band), by a shift that floating point adds exactly: the offsets stay what they were
    shift = np.array([-2.625, 1.21875])
    a[:, :2] += shift
    b[:, :2] += shift
    inside = ((b[:, :2] > w.lb[:2]) & (b[:, :2] < w.ub[:2])).all(axis=1)
    a, b = a[inside], b[inside]
    P = O.rs_connect(a, b, 1.0)
    assert (P["length"] == 0.0).sum() >= 20
    assert ((P["motion_length"][:, 0] == 0.0) & (P["length"] > 0.0)).sum() >= 100  # paths that start with a zero-length motion
    gv, gl = val.is_rs_path_valid(P)
    wv, wl = O.rs_paths_valid(w, P)
    print("structured paths on the 256 map: %d, valid share %.3f, mismatching verdicts %d, last ratios %d" % (len(P), wv.mean(), (gv != wv).sum(), (gl != wl).sum()))
    assert 0.05 < wv.mean() < 0.95
    assert np.array_equal(gv, wv) and np.array_equal(gl, wl)
    g = R.Grid(w)
    fp = pa.Footprint(ms, R.CAR3)
    sub = P[::3]
    v_want, l_want, guard, _ = R.fp_rs_paths(g, sub, R.CAR3)
    assert 0.05 < v_want.mean() < 0.95
    assert (sub["length"] == 0.0).sum() >= 5 and ((sub["motion_length"][:, 0] == 0.0) & (sub["length"] > 0.0)).sum() >= 30
    v, l = val.is_rs_path_valid(sub, footprint=fp)
    assert_equal_outside_guard(guard, (v, v_want), (l, l_want))


# ------------------------------------------------------------------------- d: the argmin forms inside a search --
@pytest.fixture(scope="module")
def world():
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    starts, goals = S.query_candidates(lambda p: w.is_state_valid(p).astype(bool), S.N_QUERY_CANDIDATES)
    seeds = np.arange(len(starts), dtype=np.uint64) + S.QUERY_SEED0
    # the oracle on the device's own non-holonomic table, as every search parity test here; the selection itself is the oracle's alone
    planner = pa.HybridAStarBatch(val, pa.HybridAStarSearchParameters(), max_batch=4, max_nodes=32768)
    planner.initialize()
    table = planner.nonholo_table()
    planner.close()
    h = O.Hybrid(w, O.params_array(), table=table)
    kept, want = S.stable_queries(h, starts, goals, seeds)
    print("structured search queries: %d of %d candidates kept" % (len(kept), len(starts)))
    assert all(r["status"] == 0 and r["path_kind"][-1] == 2 for r in want)
    ties = S.assert_queries_exercise_the_attempt(want, goals[kept])
    return dict(w=w, ms=ms, val=val, ctx=ctx, table=table, starts=starts[kept], goals=goals[kept], seeds=seeds[kept], want=want, tie=int(np.flatnonzero(ties)[0]))


def assert_final_words(planner, want):
    for q, r in enumerate(want):
        path = planner.get_path_of(q)
        assert path["kind"][-1] == 2 and path["prim"][-1] == r["path_rsword"][-1], (q, path["prim"][-1], r["path_rsword"][-1])


def test_search_one_wave_kernel_on_structured_queries(world, monkeypatch):
    monkeypatch.setenv("PP_SEARCH_ROWS", "0")
    starts, goals, seeds = world["starts"], world["goals"], world["seeds"]
    planner, res, h = run_pair(world["w"], world["ms"], world["val"], {}, starts, goals, seeds, table=world["table"])
    assert planner.search_rows == 0
    assert compare(planner, res, h, starts, goals, seeds) == len(starts)
    assert_final_words(planner, world["want"])


def test_search_rows_kernel_on_structured_queries(world, monkeypatch):
    monkeypatch.setenv("PP_SEARCH_ROWS", "1")
    starts, goals, seeds = world["starts"], world["goals"], world["seeds"]
    planner, res, h = run_pair(world["w"], world["ms"], world["val"], {}, starts, goals, seeds, table=world["table"], search_rows=8)
    assert planner.search_rows == 8
    assert compare(planner, res, h, starts, goals, seeds) == len(starts)
    assert_final_words(planner, world["want"])
    k = min(world["tie"], len(starts) - 3)
    for n in (1, 2, 3):  # a single wave with three, two and one idle rows, from the first query whose last edge is an exact tie
        s, g, sd = starts[k:k + n], goals[k:k + n], seeds[k:k + n]
        planner, res, h = run_pair(world["w"], world["ms"], world["val"], {}, s, g, sd, table=world["table"], search_rows=4)
        assert compare(planner, res, h, s, g, sd) == n
        assert_final_words(planner, world["want"][k:k + n])


def test_search_pipeline_on_structured_queries(world):
    import pathplanning_amd as pa
    starts, goals, seeds, want = world["starts"], world["goals"], world["seeds"], world["want"]
    pipe = pa.HybridAStarPipeline(world["val"], capacity=16, max_nodes=32768, search_rows=8, log_expansions=True)  # every slot is recycled
    pipe.initialize(world["table"])
    h = O.Hybrid(world["w"], O.params_array(), table=world["table"])
    solved = []

    def inspect(q, ticket, r):
        solved.append(check_against_oracle(pipe, ticket, r, h, starts[q], goals[q], seeds[q]))
        path = pipe.get_path_of(ticket)
        assert path["kind"][-1] == 2 and path["prim"][-1] == want[q]["path_rsword"][-1], (q, path["prim"][-1], want[q]["path_rsword"][-1])

    run_pipe(pipe, starts, goals, seeds, chunk=7, logged=True, inspect=inspect)
    assert len(solved) == len(starts) and all(solved)
    pipe.close()


def test_search_footprint_rows_on_structured_queries(world):
    """the structured queries that are valid for the three-disc car through k_hybrid_search_rows_footprint<true>, against the one-wave
    footprint search query by query (the yardstick of tests/test_gpu_search_rs_call.py), every edge re-marched with the restatement"""
    import pathplanning_amd as pa
    w, ms, val = world["w"], world["ms"], world["val"]
    g = R.Grid(w)
    discs = R.CAR3
    params = pa.HybridAStarSearchParameters()
    _, curv, direc = params.primitives()

    def car_valid(p):
        ok, _, _, guard = R.fp_state(g, p, discs)
        return ok & ~guard

    starts, goals = S.query_candidates(car_valid, 22, span=9)
    n = len(starts)
    assert n >= 16 and n % 4 != 0, n
    seeds = np.arange(n, dtype=np.uint64) + S.QUERY_SEED0
    planner = pa.HybridAStarBatch(val, params, max_batch=n, max_nodes=32768)
    assert planner.search_rows == 0
    planner.initialize(world["table"])
    fp = pa.Footprint(ms, discs)
    planner.set_footprint(fp)
    want = yardstick(planner, starts, goals, seeds)
    assert sum(d["n_rs_attempts"] > 0 for d in want) >= 12 and sum(d["status"] == 0 and d["path"]["kind"][-1] == 2 for d in want) >= 8
    pipe = pa.HybridAStarPipeline(val, params, capacity=16, max_nodes=32768, search_rows=8, log_expansions=True)
    pipe.initialize(world["table"])
    pipe.set_footprint(fp)
    got, _ = run_pipe(pipe, starts, goals, seeds, chunk=7, logged=True)
    for q in range(n):
        assert_is_the_one_wave_search(got[q], want[q], q)
        if got[q]["status"] == 0:
            p = got[q]["path"]
            v, gd = edges_valid(g, discs, curv, direc, p["poses"][:-1], goals[q], plan_actions(p), p["length"][1:])
            assert v[~gd].all(), (q, np.flatnonzero(~v & ~gd))
    pipe.close()
    planner.close()
