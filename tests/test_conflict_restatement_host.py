"""CPU: the numpy restatement of a conflict call (tests/conflict_restatement.py), which tests/test_gpu_pipeline_conflicts.py compares the kernels
with, run alone on the ORACLE's plans of that file's queries (the scene of tests/test_locate_restatement_host.py: synthetic_world(256, 14, 3),
validator (1.0, 0.1), the 48 query pairs of RandomState(7)) with the profiles of tests/speed_restatement.py.  Checked without a GPU:
 - a plan against itself with equal starts conflicts at every time, with separation -2 R;
 - starts further apart than the durations give status 2 with the hold flags off, and hold_after turns that into a conflict at the shared goal-side
   standstill only where the goals are within reach;
 - trajectories move forward along the plan, stand during a dwell, and enter / leave where the record says;
 - over the margins and starts the GPU test uses, the restatement alone leaves at most footprint_ref.MAX_LEFT_OUT of the pair-times undecided, and the
   scene gives that test what its assertions need (conflicts, pairs without one, pairs never both present, a negative start)."""
import math

import numpy as np

import conflict_restatement as CR
import footprint_ref as FR
import speed_restatement as V
from test_locate_restatement_host import N, scene

POINT = [(0.0, 0.0, 1.0)]  # the point validator of the scene's maps (min_safe_radius 1.0) seen as a disc
MARGINS = (0.5, 0.2, 1.0)  # what the GPU test uses
LIM = V.limits(spacing=0.25, dwell=0.5)


def starts_of(n):
    """the start times the GPU test uses: n values between -3 s and 9 s, a negative one among them, none on a lattice point of 0.1 s or 0.05 s"""
    return np.round(np.random.RandomState(11).uniform(-3.0, 9.0, n), 3) + 0.0123


_PROFILES = {}


def profiles(lim=LIM):
    key = tuple(sorted(lim.items()))
    if key not in _PROFILES:
        plans = scene()[0]
        out = []
        for p in plans:
            prof = V.profile(p, lim)
            out.append(np.column_stack([prof["s"], prof["v"], prof["t"]]) if prof["status"] == 0 else None)
        _PROFILES[key] = (plans, out)
    return _PROFILES[key]


def test_a_plan_against_itself_and_starts_further_apart_than_the_durations():
    plans, rows = profiles()
    checked = 0
    for q in range(N):
        if plans[q] is None or not plans[q].edges:
            continue
        duration = float(rows[q][-1, 2])
        kw = dict(t_from=0.0, t_to=duration + 5.0, dt=0.1, margin=0.0)
        tau, traj, (rec,) = CR.conflicts([plans[q], plans[q]], [rows[q], rows[q]], [1.0, 1.0], [(0, 1)], POINT, LIM["a_acc"], LIM["a_dec"], **kw)
        assert rec["status"] == 1 and rec["n_conflict"] == rec["n_times"] == traj[0]["n_present"] > 0 and rec["min_separation"] == -2.0
        assert (rec["separation"] == -2.0).all() and rec["t_first"] == rec["t_min"] == tau[traj[0]["first"]] and rec["undecided"] == 0
        # the same plan started later than the first one's duration: never both present; held behind its end: the two stand... a plan's length apart
        apart = [1.0, 1.0 + duration + 0.35]
        _, _, (rec,) = CR.conflicts([plans[q], plans[q]], [rows[q], rows[q]], apart, [(0, 1)], POINT, LIM["a_acc"], LIM["a_dec"], **dict(kw, t_to=2.0 * duration + 5.0))
        assert rec["status"] == 2 and rec["n_times"] == 0 and rec["min_separation"] == math.inf
        _, held, (rec,) = CR.conflicts([plans[q], plans[q]], [rows[q], rows[q]], apart, [(0, 1)], POINT, LIM["a_acc"], LIM["a_dec"], hold_after=True,
                                       **dict(kw, t_to=2.0 * duration + 5.0))
        assert rec["n_times"] == held[1]["n_present"] > 0 and rec["status"] == 1  # the second arrives where the first stands
        assert rec["min_separation"] == -2.0 and rec["t_min"] > apart[1]
        checked += 1
    assert checked >= 40


def test_hold_after_conflicts_only_where_the_goals_are_within_reach():
    plans, rows = profiles()
    solved = [q for q in range(N) if plans[q] is not None and plans[q].edges]
    near = far = 0
    for a, b in zip(solved[:-1], solved[1:]):
        da, db = float(rows[a][-1, 2]), float(rows[b][-1, 2])
        t_start = [0.0, da + 1.05]  # b starts after a has arrived
        kw = dict(t_from=0.0, t_to=da + db + 3.0, dt=0.1, margin=0.3)
        _, _, (off,) = CR.conflicts([plans[a], plans[b]], [rows[a], rows[b]], t_start, [(0, 1)], POINT, LIM["a_acc"], LIM["a_dec"], **kw)
        _, traj, (on,) = CR.conflicts([plans[a], plans[b]], [rows[a], rows[b]], t_start, [(0, 1)], POINT, LIM["a_acc"], LIM["a_dec"], hold_after=True, **kw)
        assert off["status"] == 2 and on["n_times"] == traj[1]["n_present"]
        # a stands at its goal all the while: the pair conflicts iff b's path comes within 2 R + margin of a's goal pose
        goal = traj[0]["poses"][traj[0]["last"]]
        reach = np.hypot(*(traj[1]["poses"][traj[1]["present"]][:, :2] - goal[:2]).T).min() - 2.0
        if abs(reach - 0.3) > 1e-6:
            assert (on["status"] == 1) == (reach < 0.3), (a, b, reach)
            near += on["status"] == 1
            far += on["status"] == 0
    print("%d pairs within reach of the standing vehicle, %d not" % (near, far))
    assert far >= 10 and near + far >= 30


def test_trajectories_move_forward_stand_for_a_dwell_and_enter_where_the_record_says():
    lim = V.limits(spacing=0.25, dwell=1.5)
    plans, rows = profiles(lim)
    dwelt = 0
    for q in range(N):
        if rows[q] is None:
            continue
        tau = CR.times(*CR.lattice(-1.0, float(rows[q][-1, 2]) + 1.0, 0.05), 0.05)
        tr = CR.trajectory(plans[q], rows[q], 0.0, tau, lim["a_acc"], lim["a_dec"])
        k = np.flatnonzero(tr["present"])
        assert tr["status"] == 0 and (k == np.arange(k[0], k[-1] + 1)).all() and tau[k[0]] >= 0.0 and tau[k[-1]] <= rows[q][-1, 2]
        assert (np.diff(tr["s"][k]) >= 0.0).all() and tr["s_enter"] == tr["s"][k[0]] and tr["s_leave"] == tr["s"][k[-1]] and np.isnan(tr["poses"][~tr["present"]]).all()
        assert abs(tr["s_leave"] - plans[q].length) <= 5.0 * 0.05 + 1e-9 and tr["s_enter"] == 0.0
        hold = CR.trajectory(plans[q], rows[q], 0.0, tau, lim["a_acc"], lim["a_dec"], True, True)
        assert hold["n_present"] == len(tau) and hold["s_enter"] == 0.0 and hold["s_leave"] == rows[q][-1, 0]
        for j in np.flatnonzero((np.diff(rows[q][:, 0]) == 0.0) & (np.diff(rows[q][:, 2]) >= 1.5)):
            inside = (tau >= rows[q][j, 2]) & (tau <= rows[q][j + 1, 2])
            assert inside.sum() >= 29 and (tr["s"][inside] == rows[q][j, 0]).all() and (tr["poses"][inside] == tr["poses"][inside][0]).all()
            dwelt += 1
    assert dwelt >= 1


def test_the_share_of_undecided_pair_times_is_within_the_cap_and_the_scene_has_what_the_gpu_cases_need():
    plans, rows = profiles()
    t_start = starts_of(N)
    assert (t_start < 0).any() and not np.isclose(np.round(t_start / 0.05), t_start / 0.05, atol=1e-6).any()
    times = undecided = 0
    for margin in MARGINS:
        for hold in ((False, False), (True, True)):
            kw = dict(t_from=0.0, t_to=12.95, dt=0.1, margin=margin, hold_before=hold[0], hold_after=hold[1])
            tau, traj, recs = CR.conflicts(plans[:N], rows[:N], t_start, None, POINT, LIM["a_acc"], LIM["a_dec"], **kw)
            assert len(tau) == 130 and len(recs) == 1128
            times += sum(r["n_times"] for r in recs)
            undecided += sum(r["undecided"] for r in recs)
            status = [r["status"] for r in recs]
            print("margin %g hold %s: %d conflicts, %d without, %d never both present, %d without a plan" % (margin, hold, status.count(1), status.count(0), status.count(2), status.count(-1)))
            assert status.count(1) >= 3 and status.count(0) >= 100 and status.count(-1) >= 47
            assert hold[0] or status.count(2) >= 1
    print("%d pair-times, %d undecided" % (times, undecided))
    assert times >= 100000 and undecided <= FR.MAX_LEFT_OUT * times
    for discs in (FR.CAR3,):
        kw = dict(t_from=0.0, t_to=9.9, dt=0.15, margin=MARGINS[1], hold_after=True)
        _, _, recs = CR.conflicts(plans[:24], rows[:24], starts_of(24) * 0.5, None, discs, LIM["a_acc"], LIM["a_dec"], **kw)
        n, u = sum(r["n_times"] for r in recs), sum(r["undecided"] for r in recs)
        assert u <= FR.MAX_LEFT_OUT * n
