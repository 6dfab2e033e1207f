"""The preconditions of tests/test_gpu_rs_structured.py, checked on the CPU oracle alone, so that the device tests cannot pass on an empty
set: the structured pose pairs (tests/rs_structured.py) do contain the knife-edge inputs -- words that a one-ulp nudge flips (but few enough
that the unflagged rest is a strict test), motions of length exactly 0 and nearly 0, zero-length paths, cusps at ratio 0 and 1, every word
family, exact float-cost ties between a word and its mirror image -- and the oracle's paths on them reach their goals, by an integration of
the path records that shares no code with the oracle."""
import numpy as np
import pytest

import oracle_lib as O
import rs_structured as S

RMIN = 2.0
# oracle end pose against the longdouble integration of its own record and against the goal.  Coordinates reach 8 * rmin + 7 = 23 (one ulp:
# 3.6e-15); a record chains at most five motions of a handful of roundings and two 1-ulp libm calls each, and the solver's t, u, v carry a
# few ulp of an angle that a lever of up to 23 m turns into position: some tens of ulp(23) in all.  300 ulp(23) = 1e-12 bounds that.
END_POSE_TOL = 1e-12


@pytest.fixture(scope="module")
def pairs():
    return S.structured_pairs(RMIN)


@pytest.mark.parametrize("costs", S.COSTS)
def test_structured_set_holds_the_knife_edge_inputs(pairs, costs):
    a, b = pairs
    n = len(a)
    assert n == S.N_GRID + S.N_UNWRAPPED + S.N_NEAR_OFFSET
    mask, seen = S.flagged(a, b, RMIN, costs)
    assert 0 < mask.mean() < 0.03, mask.mean()  # fragile pairs exist, and the strict comparison covers more than 97 %
    assert (seen.sum(axis=1) >= 1).all() and np.array_equal(seen.sum(axis=1) > 1, mask)
    word, tuv, cost, seg = O.rs_optimal_batch(a, b, RMIN, *costs)
    P = O.rs_connect(a, b, RMIN, *costs)
    assert np.array_equal(P["word"], word)
    zero, tiny = S.zero_or_tiny(P)
    assert zero.mean() >= 0.02 and tiny.mean() >= 0.005, (zero.mean(), tiny.mean())
    assert (P["length"] == 0.0).sum() >= 20
    cusps = O.rs_path_cusps(P)
    count = np.array([len(c) for c in cusps])
    assert sum(1 for c in cusps if len(c) and ((c == 0.0).any() or (c >= 1.0).any())) >= 30
    assert (np.bincount(count, minlength=3)[:3] > 0).all()
    assert set(np.unique(word // 4)) == set(range(12))
    ties = S.mirror_ties(a, b, RMIN, costs, word, cost) & ~mask
    print("costs %s: flagged %.4f (%d), zero motion %.4f, tiny %.4f, zero-length %d, cusp counts %s, unflagged exact ties %d"
          % (costs, mask.mean(), mask.sum(), zero.mean(), tiny.mean(), (P["length"] == 0.0).sum(), np.bincount(count).tolist(), ties.sum()))
    assert ties.sum() >= 200


@pytest.mark.parametrize("costs", S.COSTS)
def test_oracle_paths_reach_their_goals_by_independent_integration(pairs, costs):
    a, b = pairs
    P = O.rs_connect(a, b, RMIN, *costs)
    zero, tiny = S.zero_or_tiny(P)
    end = S.integrate_records(P, must=zero | tiny | S.flagged(a, b, RMIN, costs)[0] if not S.LONGDOUBLE_OK else None)
    assert S.LONGDOUBLE_OK or np.isfinite(np.asarray(end, np.float64)[zero | tiny]).all()
    e_own = S.pose_error(end, P["final_pose"])
    e_goal = S.pose_error(end, b)
    e_final = S.pose_error(P["final_pose"], b)
    print("costs %s: oracle final_pose vs integrate %.3g, integrate vs goal %.3g, final_pose vs goal %.3g" % (costs, e_own.max(), e_goal.max(), e_final.max()))
    assert max(e_own.max(), e_goal.max(), e_final.max()) < END_POSE_TOL
    # the reported length is the sum of the motions
    used = (P["direction"] != S.NO_MOTION) & np.isfinite(P["motion_length"])
    assert np.array_equal(P["length"], S.record_length(P, used))


def test_integrate_on_hand_made_records():
    """integrate() itself: quarter turns, a straight and a reversal, against poses known by construction"""
    half_pi = np.pi / 2
    recs = [  # steer, direction, motion_length (angle / length in radii), start, rmin, end
        ([S.LEFT], [S.FORWARD], [half_pi], (0, 0, 0), 2.0, (2, 2, half_pi)),
        ([S.RIGHT], [S.FORWARD], [half_pi], (0, 0, 0), 2.0, (2, -2, -half_pi)),
        ([S.LEFT], [S.BACKWARD], [half_pi], (0, 0, 0), 2.0, (-2, 2, -half_pi)),
        ([S.RIGHT], [S.BACKWARD], [half_pi], (0, 0, 0), 2.0, (-2, -2, half_pi)),
        ([S.STRAIGHT], [S.BACKWARD], [1.5], (1, 1, half_pi), 2.0, (1, -2, half_pi)),
        ([S.LEFT, S.STRAIGHT, S.RIGHT], [S.FORWARD, S.FORWARD, S.FORWARD], [half_pi, 1.0, half_pi], (1, -1, 0), 1.0, (3, 2, 0)),
        ([S.LEFT, S.STRAIGHT], [S.FORWARD, S.FORWARD], [0.0, 0.0], (4, 5, 0.3), 1.0, (4, 5, 0.3)),
    ]
    for steer, direction, length, start, rmin, want in recs:
        k = len(steer)
        st = np.array([steer + [0] * (5 - k)], dtype=np.int8)
        di = np.array([direction + [S.NO_MOTION] * (5 - k)], dtype=np.int8)
        ln = np.array([length + [np.inf] * (5 - k)])
        got = S.integrate(np.array([start], dtype=np.float64), st, di, ln, rmin, must=np.ones(1, bool))
        assert S.pose_error(got, np.array([want], dtype=np.float64)).max() < 1e-15 * 8, (steer, direction, got)


def test_junction_ratios_sit_on_the_selections():
    a, b = S.structured_pairs(RMIN)
    P = O.rs_connect(a[::7], b[::7], RMIN, 2.0, 1.0, 0.5)
    J = S.junction_ratios(P)
    assert J.shape == (len(P), 17) and np.isfinite(J).all()
    assert (J[:, 15] == 0.0).all() and (J[:, 16] == 1.0).all()
    live = P["length"] > 0
    assert np.array_equal(J[live, 1], np.nextafter(J[live, 0], np.inf)) and np.array_equal(J[live, 2], np.nextafter(J[live, 0], -np.inf))
    assert np.array_equal(J[live, 0], P["motion_length"][live, 0] * RMIN / P["length"][live])
    # the direction the oracle reports changes across a junction between two motions of different direction
    two = live & (P["direction"][:, 1] != S.NO_MOTION) & (P["direction"][:, 1] != P["direction"][:, 0]) & (P["motion_length"][:, 0] > 1e-6) & (P["motion_length"][:, 1] > 1e-6)
    assert two.sum() > 100
    below = O.rs_path_interpolate(P[two], J[two, 2])[1]
    above = O.rs_path_interpolate(P[two], J[two, 0] + 1e-9)[1]
    assert np.array_equal(below, P["direction"][two, 0]) and np.array_equal(above, P["direction"][two, 1])
    # ... and one float above the junction the product ratio * length decides either way: the knife edge these ratios are for
    edge = O.rs_path_interpolate(P[two], J[two, 1])[1]
    assert (edge == P["direction"][two, 0]).any() and (edge == P["direction"][two, 1]).any()


def test_structured_search_queries_are_reproducible_on_the_oracle():
    """the selection of tests/test_gpu_rs_structured.py's search queries with the oracle's own non-holonomic table: enough of the
    structured candidates keep status, expansion count, attempts and plan under every one-ulp nudge, and the kept ones exercise the
    Reeds-Shepp attempt (one-edge plans, rejected attempts)"""
    w = O.synthetic_world(256, 6, 3)
    table, _ = O.nonholo_build(w.lb, w.ub)
    h = O.Hybrid(w, O.params_array(), table=table)
    starts, goals = S.query_candidates(lambda p: w.is_state_valid(p).astype(bool), S.N_QUERY_CANDIDATES)
    seeds = np.arange(len(starts), dtype=np.uint64) + S.QUERY_SEED0
    kept, res = S.stable_queries(h, starts, goals, seeds)
    print("structured search queries: %d of %d candidates kept" % (len(kept), len(starts)))
    S.assert_queries_exercise_the_attempt(res, goals[kept])
