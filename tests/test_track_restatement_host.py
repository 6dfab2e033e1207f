"""CPU: the numpy restatement of a delay call with tracked movers (tests/track_restatement.py), which tests/test_gpu_pipeline_deconflict_tracks.py
compares the kernels with, run alone on the ORACLE's plans of that file's queries (the scene of tests/test_conflict_restatement_host.py) with the
profiles of tests/speed_restatement.py.  CASES are the GPU test's cases by name; the tracks of a case are built from the scene by tracks_of():
 - a follower: a plan's own restated trajectory, resampled every 0.5 s and shifted in time;
 - a crosser on a straight line between two start poses;
 - a stander, two waypoints at a plan's goal: once for part of the horizon, once for the whole of it;
 - a track that begins and one that ends in the middle of the horizon;
 - a one-waypoint track on an exact lattice time, where a vehicle is at that time;
 - radii 0, 0.3 and 1.0.
Checked without a GPU: the restatement alone leaves NO vehicle undecided in any case; without tracks it gives tests/delay_restatement.py's records;
every scheduled vehicle's track records have status 0 or 2; every vehicle whose blocker is a track conflicts with that track one step earlier, where
its record says (by a route that shares nothing with track_restatement: np.interp on the waypoints); and the cases hold what the GPU test's
assertions need -- vehicles that wait for a track, status 1 from a stander, a track blocker and a vehicle blocker in one call, status -1."""
import numpy as np

import conflict_restatement as CR
import delay_restatement as DR
import track_restatement as TR
from test_conflict_restatement_host import LIM, profiles
from test_delay_restatement_host import HOLDS, TS
from test_delay_restatement_host import cases as delay_cases
from test_locate_restatement_host import scene

DS = (0, 1, 64, 65)
MS = (1, 3, 17)
RADII = (0.3, 1.0, 0.0)
NAMES = (["T=%d" % T for T in TS] + ["D=%d" % D for D in DS] + ["M=%d" % M for M in MS] + ["no pairs", "chain", "star"] + ["nearest, " + h for h in HOLDS] + ["CAR3"])


def cases(starts):
    """the calls of the GPU test by name: tests/test_delay_restatement_host.py's (which plans, pair list or None, start times, discs, keywords of the
    call), and how many tracks of tracks_of() go with them"""
    base = delay_cases(starts)
    out = {}
    for T in TS:
        out["T=%d" % T] = base["T=%d" % T] + (3,)
    for D in DS:
        out["D=%d" % D] = base["D=%d" % D] + (3,)
    for M in MS:
        out["M=%d" % M] = base["all-12"] + (M,)
    which, _, t_start, discs, kw = base["all-12"]
    out["no pairs"] = (which, [], t_start, discs, kw, 7)
    out["chain"] = base["chain"] + (7,)
    out["star"] = base["star"] + (7,)
    for h in HOLDS:
        out["nearest, " + h] = base["nearest, " + h] + (3,)
    out["CAR3"] = base["CAR3"] + (7,)
    assert list(out) == NAMES
    return out


def rounded(rows):
    """waypoints to the micrometre and microsecond: the oracle's plans and the device's give the same tracks"""
    return np.round(np.asarray(rows, dtype=np.float64).reshape(-1, 3), 6)


def tracks_of(plans, rows, starts, goals, which, t_start, kw, M):
    """M tracks [(radius, waypoints [W, 3])] for a call over the plans `which` (indices into plans, rows, starts, goals) with the start times t_start and
    the keywords kw, built from the scene alone.  The kinds repeat in the order follower, one-waypoint, stander for a part, crosser, stander for the whole,
    beginning, ending; the radii cycle through RADII."""
    k0, T = CR.lattice(kw["t_from"], kw["t_to"], kw["dt"])
    tau = CR.times(k0, T, kw["dt"])
    t0, t1, dt = float(tau[0]), float(tau[-1]), float(kw["dt"])
    D = int(kw.get("max_delay_steps", 0))
    solved = [i for i, q in enumerate(which) if plans[q] is not None and rows[q] is not None and len(rows[q]) and plans[q].edges]
    assert len(solved) >= 4
    starts, goals = np.asarray(starts, dtype=np.float64), np.asarray(goals, dtype=np.float64)
    out = []
    for k in range(M):
        kind, turn = k % 7, k // 7
        i = solved[(3 * k + turn) % len(solved)]
        j = solved[(3 * k + turn + 1) % len(solved)]
        q, R = which[i], RADII[k % 3]
        duration = float(rows[q][-1, 2])
        if kind == 0:  # a follower: the plan's own trajectory 1.2 s (and more each turn) behind the vehicle's undelayed timetable
            u = np.append(np.arange(0.0, duration, 0.5), duration)
            _, s = CR.position(rows[q], u, LIM["a_acc"], LIM["a_dec"])
            xy = CR.poses_at(plans[q], s)[0][:, :2]
            w = np.column_stack([u + float(t_start[i]) + 1.2 + 0.9 * turn, xy])
        elif kind == 1:  # one waypoint on an exact lattice time, where vehicle i is then on its undelayed timetable (else at its start pose)
            m = min(T - 1, max(0, int(np.ceil((float(t_start[i]) + 0.4 * duration - t0) / dt))))
            _, s = CR.position(rows[q], np.array([tau[m] - np.float64(t_start[i])]), LIM["a_acc"], LIM["a_dec"])
            w = np.array([[tau[m], *CR.poses_at(plans[q], s)[0][0, :2]]])
        elif kind == 2:  # a stander at vehicle i's goal while the undelayed vehicle arrives, gone a little later
            arrive = float(t_start[i]) + duration
            w = np.array([[arrive - 2.0, *goals[q][:2]], [arrive + 0.15 * dt * min(D, 40) + 0.35 * dt, *goals[q][:2]]])
        elif kind == 3:  # a crosser on the straight line between two start poses, at 2 m/s from the first lattice time on
            a, b = starts[q][:2], starts[which[j]][:2]
            w = np.array([[t0 - 0.03, *a], [t0 - 0.03 + max(float(np.hypot(*(b - a))) / 2.0, 0.5), *b]])
        elif kind == 4:  # a stander at vehicle i's goal for the whole horizon and beyond
            w = np.array([[t0 - 1.0, *goals[q][:2]], [t1 + 1.0, *goals[q][:2]]])
        elif kind == 5:  # begins in the middle of the horizon (between two lattice times) and drives from a goal to a start
            begin = 0.5 * (t0 + t1) + 0.37 * dt
            w = np.array([[begin, *goals[q][:2]], [begin + 4.0, *starts[which[j]][:2]], [begin + 9.0, *starts[q][:2]]])
        else:  # ends in the middle of the horizon
            end = 0.5 * (t0 + t1) - 0.41 * dt
            w = np.array([[end - 7.5, *starts[q][:2]], [end - 3.0, *goals[which[j]][:2]], [end, *goals[q][:2]]])
        w = rounded(w)
        if kind == 1:
            w[0, 0] = tau[m]  # (the lattice time's own bits)
        assert (np.diff(w[:, 0]) > 0).all()
        out.append((R, w))
    return out


def shifted_centres(t, discs, D, d, T):
    """the disc centres [K, T, 2] and presence of a vehicle delayed by d steps: the columns m + D - d of its extended trajectory"""
    c = np.arange(T) + D - d
    return CR.centres(np.nan_to_num(t["poses"][c]), discs), t["present"][c], t["s"][c]


def check_schedule(tau, traj, recs, track_recs, tracks, discs, kw):
    """independent of track_restatement.decide: the position of a track is np.interp's.  Every scheduled vehicle is clear of every track and its records
    say so; a vehicle whose blocker is a track conflicts with it at the last rejected candidate, first at t_block, where s_block says"""
    T, D, n = len(tau), kw["max_delay_steps"], len(recs)
    radius = [np.float64(np.float32(r)) for _, _, r in discs]
    for i, r in enumerate(recs):
        assert len(track_recs[i]) == len(tracks)
        if r["status"] < 0:
            assert all(t["status"] == -1 for t in track_recs[i])
            continue
        assert r["n_tried"] == (r["delay_steps"] + 1 if r["status"] == 0 else D + 1)
        for d, want_clear in ((r["delay_steps"], True), (r["delay_steps"] - 1 if r["status"] == 0 else D, False)):
            if d < 0 or (want_clear and r["status"] != 0):
                continue
            centre, present, s = shifted_centres(traj[i], discs, D, d, T)
            first = {}
            for k, (R, w) in enumerate(tracks):
                there = present & (tau >= w[0, 0]) & (tau <= w[-1, 0])
                x, y = np.interp(tau, w[:, 0], w[:, 1]), np.interp(tau, w[:, 0], w[:, 2])
                sep = np.min([np.hypot(centre[a, :, 0] - x, centre[a, :, 1] - y) - (radius[a] + R) for a in range(len(discs))], axis=0)
                hit = np.flatnonzero(there & (sep < kw["margin"]))
                if want_clear:
                    rec = track_recs[i][k]
                    assert not len(hit) and rec["status"] in (0, 2) and rec["n_conflict"] == 0 and rec["n_times"] == int(there.sum()), (i, k, rec)
                    if rec["status"] == 0:
                        assert abs(rec["min_separation"] - sep[there].min()) < 1e-9 and rec["min_separation"] >= kw["margin"]
                elif len(hit):
                    first[k] = int(hit[0])
            if not want_clear and r["blocker"] >= n:
                k = r["blocker"] - n
                assert k in first and tau[first[k]] == r["t_block"] and r["s_block"] == (float(s[first[k]]), 0.0), (i, k, r)
                assert all(m >= first[k] and (m > first[k] or other >= k) for other, m in first.items())  # the least key among the tracks
                if r["status"] == 1:  # the reported candidate is the rejected one: the record tells the same
                    rec = track_recs[i][k]
                    assert rec["status"] == 1 and rec["t_first"] == r["t_block"] and rec["s_first"] == r["s_block"][0]


def test_without_tracks_the_records_are_the_delay_restatements():
    plans, rows = profiles()
    starts = scene()[1]
    for name in ("T=65", "D=64", "chain", "nearest, hold-both"):
        which, pairs, t_start, discs, kw, _ = cases(starts)[name]
        call = ([plans[q] for q in which], [rows[q] for q in which], t_start, pairs, discs, LIM["a_acc"], LIM["a_dec"])
        _, _, want = DR.deconflict(*call, **kw)
        _, _, got, track_recs = TR.deconflict_tracks(*call, None, **kw)
        assert got == want and all(r == [] for r in track_recs), name


def test_over_the_gpu_cases_no_vehicle_is_undecided_and_every_schedule_holds():
    plans, rows = profiles()
    _, starts, goals, _ = scene()
    waited_for_track = stander_blocks = without = mixed = 0
    kinds = set()
    for name, (which, pairs, t_start, discs, kw, M) in cases(starts).items():
        tracks = tracks_of(plans, rows, starts, goals, which, t_start, kw, M)
        assert len(tracks) == M and {R for R, _ in tracks} == set(RADII[:min(M, 3)])
        tau, traj, recs, track_recs = TR.deconflict_tracks([plans[q] for q in which], [rows[q] for q in which], t_start, pairs, discs, LIM["a_acc"], LIM["a_dec"], tracks, **kw)
        n = len(which)
        status = [r["status"] for r in recs]
        by_track = [r for r in recs if r["blocker"] >= n]
        by_vehicle = [r for r in recs if 0 <= r["blocker"] < n]
        print("%s: %d tracks, %d scheduled (%d waited, longest %d), %d blocked, %d without a plan; blocker a track %d, a vehicle %d; %d undecided" % (
            name, M, status.count(0), sum(r["delay_steps"] > 0 for r in recs), max(r["delay_steps"] for r in recs), status.count(1), status.count(-1),
            len(by_track), len(by_vehicle), sum(r["undecided"] for r in recs)))
        assert not any(r["undecided"] for r in recs), name
        assert not any(t["undecided"] for row in track_recs for t in row), name
        check_schedule(tau, traj, recs, track_recs, tracks, discs, kw)
        waited_for_track += sum(r["status"] == 0 for r in by_track)
        stander_blocks += sum(r["status"] == 1 and (r["blocker"] - n) % 7 == 4 for r in by_track)
        without += status.count(-1)
        mixed += bool(by_track) and bool(by_vehicle)
        kinds |= {k % 7 for k in range(M)}
        if name == "no pairs":
            assert not by_vehicle and by_track
        if name == "D=0":
            assert all(r["delay_steps"] in (0, -1) and r["n_tried"] == 1 for r in recs if r["status"] >= 0)
        # absent before and behind its waypoints, and the whole-horizon stander present at every time
        for i, row in enumerate(track_recs):
            if recs[i]["status"] >= 0 and M >= 5 and traj[i]["status"] == 0:
                assert row[4]["n_times"] == max(t["n_times"] for t in row)
    assert kinds == set(range(7))
    assert waited_for_track >= 10 and stander_blocks >= 2 and without >= 4 and mixed >= 3
