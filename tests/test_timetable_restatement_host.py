"""CPU: the numpy restatement of a timetable call (tests/timetable_restatement.py), which tests/test_gpu_pipeline_timetable.py compares the kernel
with, run alone on the ORACLE's plans of that file's queries (the scene of tests/test_conflict_restatement_host.py) with the profiles of
tests/speed_restatement.py.  Checked without a GPU:
 - t(s) never decreases in s, and s(t(s)) is s within the suite's TOL of 1e-9 m (the measured worst value is printed);
 - the by-time arc length is conflict_restatement.position's, bit for bit;
 - every stop has t_arrive <= t_depart, and at a cusp stop the two differ by the dwell within 1e-12;
 - next_stop is -1 exactly for the look-ups whose row is at or behind the last listed stop's row;
 - edge and ratio come back from the pose for DECIDED look-ups, and the undecided share on these plans stays within footprint_ref.MAX_LEFT_OUT: the
   condition under which the GPU file uses the same cap."""
import numpy as np

import conflict_restatement as CR
import footprint_ref as FR
import test_conflict_restatement_host as CH
import timetable_restatement as TT

TOL = 1e-9
LIM = CH.LIM  # spacing 0.25, dwell 0.5: what the GPU test uses
N = CH.N


def solved():
    plans, rows = CH.profiles()
    return [(q, plans[q], rows[q]) for q in range(N) if rows[q] is not None]


def DWELT_PLAN():
    """the first plan with a cusp stop that dwells: the one whose mixed look-ups include its inner stops and dwells.  A cusp stop is where the direction
    changes, so its look-ups are undecided by nature; the other plans' look-ups stay off the stops so that the cap on the undecided share means something."""
    for q, plan, rows in solved():
        st = TT.stops(rows, LIM["a_acc"], LIM["a_dec"])
        if (st["t_arrive"] < st["t_depart"]).any():
            return q
    raise AssertionError("the scene has no cusp stop")


def test_time_never_decreases_along_the_plan_and_the_round_trip_returns_the_arc_length():
    worst = looked = 0
    for q, plan, rows in solved():
        s = np.sort(np.concatenate([np.random.RandomState(q).uniform(rows[0, 0], rows[-1, 0], 1500), rows[:, 0]]))
        status, j, s_out, t, v, a = TT.by_length(rows, s, LIM["a_acc"], LIM["a_dec"])
        assert (status == 0).all() and np.array_equal(s_out, s)
        assert (np.diff(t) >= 0.0).all(), q
        assert (t >= rows[j, 2]).all() and (t <= rows[np.minimum(j + 1, len(rows) - 1), 2]).all() and (v >= 0.0).all()
        _, back = CR.position(rows, t, LIM["a_acc"], LIM["a_dec"])
        worst = max(worst, float(np.abs(back - s).max()))
        looked += len(s)
        # at a row of the profile: its time and its speed (behind equal arc lengths the last row's)
        status, j, _, t, v, _ = TT.by_length(rows, rows[:, 0], LIM["a_acc"], LIM["a_dec"])
        last = np.searchsorted(rows[:, 0], rows[:, 0], side="right") - 1
        assert np.array_equal(j, last) and np.array_equal(t, rows[last, 2]) and np.array_equal(v, rows[last, 1])
    print("%d look-ups by arc length: worst |s(t(s)) - s| = %.3g m" % (looked, worst))
    assert looked > 60000 and worst <= TOL


def test_the_arc_length_by_time_is_the_conflict_calls_position():
    looked = 0
    for q, plan, rows in solved():
        u = np.concatenate([np.random.RandomState(100 + q).uniform(-1.0, rows[-1, 2] + 1.0, 1000), rows[:, 2]])
        status, j, s, t, v, a = TT.by_time(rows, u, LIM["a_acc"], LIM["a_dec"])
        present, want = CR.position(rows, u, LIM["a_acc"], LIM["a_dec"], True, True)
        assert present.all() and np.array_equal(s.view(np.uint64), want.view(np.uint64)), q
        assert np.array_equal(status, np.where(u < 0, 1, np.where(u > rows[-1, 2], 2, 0))) and np.array_equal(t, np.clip(u, 0.0, rows[-1, 2]))
        assert (v >= 0.0).all() and (v <= max(LIM["v_max_forward"], LIM["v_max_reverse"]) + 1e-9).all()
        assert (np.abs(a) <= max(LIM["a_acc"], LIM["a_dec"]) * (1.0 + 1e-9)).all()
        # at a row of the profile: its speed (behind equal times the last row's)
        last = np.searchsorted(rows[:, 2], rows[:, 2], side="right") - 1
        _, j, _, _, v, _ = TT.by_time(rows, rows[:, 2], LIM["a_acc"], LIM["a_dec"])
        assert np.array_equal(j, last) and np.array_equal(v, rows[last, 1])
        looked += len(u)
    assert looked > 40000


def test_stops_arrive_before_they_depart_and_cusp_stops_dwell():
    cusps = ends = 0
    for q, plan, rows in solved():
        st = TT.stops(rows, LIM["a_acc"], LIM["a_dec"])
        assert (st["t_arrive"] <= st["t_depart"]).all() and (np.diff(st["row"]) > 0).all()
        assert st["row"][0] == 0 and st["row"][-1] == len(rows) - 1 and st["t_arrive"][0] == 0.0  # (v_start = v_end = 0: both ends stand)
        ends += 2
        inner = st[(st["row"] > 0) & (st["row"] < len(rows) - 1)]
        # an inner stop of these profiles is a cusp stop -- possibly with its twin across a junction, which the vehicle reaches and leaves at once
        gap = inner["t_depart"] - inner["t_arrive"]
        assert (np.abs(gap[gap > 0.0] - LIM["dwell"]) < 1e-12).all()
        cusps += int((gap > 0.0).sum())
    print("%d cusp stops with a dwell, %d standing ends" % (cusps, ends))
    assert cusps >= 1


def test_next_stop_is_absent_exactly_behind_the_last_listed_stop():
    seen_cut = False
    for q, plan, rows in solved():
        for max_stops in (0, 1, 2, 16):
            values = TT.mixed_values(rows, "length", 70, LIM["a_acc"], LIM["a_dec"], seed=q)
            rec, listed, out, _ = TT.timetable(False, rows, values, "length", LIM["a_acc"], LIM["a_dec"], max_stops)
            assert rec["n_listed"] == len(listed) == min(rec["n_stops"], max_stops)
            behind = np.ones(len(out), dtype=bool) if len(listed) == 0 else out["row"] >= listed["row"][-1]
            assert np.array_equal(out["next_stop"] == -1, behind), (q, max_stops)
            k = out["next_stop"][~behind]
            assert (listed["row"][k] > out["row"][~behind]).all() and (k == 0).all() | (listed["row"][np.maximum(k - 1, 0)] <= out["row"][~behind])[k > 0].all()
            assert (out["s_to_stop"][~behind] >= 0.0).all() and (out["t_to_stop"][~behind] >= 0.0).all() and not out["s_to_stop"][behind].any()
            assert (out["t_remaining"] >= 0.0).all()
            seen_cut |= rec["n_stops"] > max_stops > 0
    assert seen_cut


def test_edge_and_ratio_return_the_pose_where_decided_and_the_undecided_share_is_within_the_cap():
    looked = undecided = 0
    dwelt = DWELT_PLAN()
    for q, plan, rows in solved():
        for by in ("length", "time"):
            values = TT.mixed_values(rows, by, 70, LIM["a_acc"], LIM["a_dec"], seed=q, stops_too=q == dwelt)
            rec, listed, out, decided = TT.timetable(plan, rows, values, by, LIM["a_acc"], LIM["a_dec"])
            looked += len(out)
            undecided += int((~decided).sum())
            if not plan.edges:
                assert not out["edge"].any() and not out["ratio"].any() and (out["pose"] == plan.first).all()
                continue
            k = np.flatnonzero(decided)
            poses, _ = plan.at(out["edge"][k], out["ratio"][k])
            assert np.abs(poses - out["pose"][k]).max() <= TOL
            assert (out["edge"] >= 1).all() and (out["edge"] <= len(plan.edges)).all() and (out["ratio"] >= 0.0).all() and (out["ratio"] <= 1.0).all()
            assert np.abs((plan.S[out["edge"] - 1] + out["ratio"] * plan.L[out["edge"] - 1]) - out["s"]).max() <= TOL
            assert set(np.unique(out["direction"])) <= {-1, 0, 1} and (out["kappa"] >= 0.0).all()
    print("%d look-ups, %d undecided" % (looked, undecided))
    assert looked >= 5000 and undecided <= FR.MAX_LEFT_OUT * looked
