"""CPU: the numpy restatement of a delay call (tests/delay_restatement.py), which tests/test_gpu_pipeline_deconflict.py compares the kernel with,
run alone on the ORACLE's plans of that file's queries (the scene of tests/test_conflict_restatement_host.py) with the profiles of
tests/speed_restatement.py.  Checked without a GPU:
 - two identical plans from the same start: the second waits d > 0 steps, is clear at d and in conflict at d - 1 with vehicle 0 (both by
   conflict_restatement.pair on the shifted trajectories, which shares nothing with delay_restatement.decide), and its record names that conflict;
 - the same with hold_after: the first stands at the goal for ever and the second gets status 1 for every D tried;
 - starts further apart than the durations: nobody waits;
 - over CASES -- the margins, starts, pair lists and lattices the GPU test uses -- the restatement alone leaves NO vehicle undecided (no separation
   of a tried candidate within 1e-9 of the margin), every scheduled pair is clear and every vehicle that waited conflicts with its blocker one step
   earlier, and the cases hold what the GPU test's assertions need (vehicles that wait, status 1, status -1, more than one level)."""
import os
import sys

import numpy as np

import conflict_restatement as CR
import delay_restatement as DR
import footprint_ref as FR
from test_conflict_restatement_host import LIM, POINT, profiles, starts_of
from test_locate_restatement_host import N, scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from bench_pipeline_conflicts import nearest_pairs  # noqa: E402  (the pair list of the conflicts tool)

TS = (1, 63, 64, 65, 130)
DS = (0, 1, 63, 64, 65)
HOLDS = {"absent": (False, False), "hold-both": (True, True), "hold-before": (True, False), "hold-after": (False, True)}


def lattice_kw(T, margin, D, **more):
    """T lattice times from the lattice point k0 = 7 on (as tests/test_gpu_pipeline_conflicts.py forms them)"""
    kw = dict(t_from=0.7 - 1e-9, t_to=0.1 * (7 + T - 1) + 0.05, dt=0.1, margin=margin, max_delay_steps=D, **more)
    assert CR.lattice(kw["t_from"], kw["t_to"], kw["dt"]) == (7, T)
    return kw


def cases(starts):
    """the calls of the GPU test by name: (which plans, pair list or None, start times, discs, keywords of the call); `starts` are the scene's start poses"""
    out = {}
    twelve, sixteen = list(range(12)), list(range(16))
    for T in TS:
        out["T=%d" % T] = (twelve, None, starts_of(12) * 0.25, POINT, lattice_kw(T, 0.5, 64, hold_before=True))
    for D in DS:
        out["D=%d" % D] = (twelve, None, starts_of(12) * 0.1, POINT, lattice_kw(130, 0.3, D))
    chain = [(i, i + 1) if i % 2 else (i + 1, i) for i in range(15)]
    out["chain"] = (sixteen, chain, starts_of(16) * 0.1, POINT, lattice_kw(130, 0.4, 65))
    out["star"] = (sixteen, [(0, i) if i % 2 else (i, 0) for i in range(1, 16)], starts_of(16) * 0.1, POINT, lattice_kw(130, 0.4, 65))
    out["all-12"] = (twelve, None, starts_of(12) * 0.1, POINT, lattice_kw(130, 0.6, 65))
    near = [tuple(int(x) for x in p) for p in nearest_pairs(np.asarray(starts)[:N], 32)]
    for name, hold in HOLDS.items():
        out["nearest, " + name] = (list(range(N)), near, starts_of(N), POINT, lattice_kw(130, 0.5, 65, hold_before=hold[0], hold_after=hold[1]))
    out["CAR3"] = (list(range(24)), None, starts_of(24) * 0.5, FR.CAR3, dict(t_from=0.0, t_to=9.9, dt=0.15, margin=0.2, hold_after=True, max_delay_steps=40))
    return out


def shifted(t, D, d, T):
    """trajectory()'s dict of a vehicle delayed by d steps: the columns m + D - d of its extended trajectory"""
    c = np.arange(T) + D - d
    return dict(status=t["status"], present=t["present"][c], poses=t["poses"][c], s=t["s"][c], decided=t["decided"][c])


def check_schedule(tau, traj, recs, pairs, discs, kw):
    """independent of delay_restatement.decide: every pair of scheduled vehicles is clear, and a vehicle that waited conflicts with its blocker one step
    earlier, where its record says"""
    T, D, n = len(tau), kw["max_delay_steps"], len(recs)
    for a, b in (CR.all_pairs(n) if pairs is None else pairs):
        if recs[a]["status"] == 0 and recs[b]["status"] == 0:
            rec = CR.pair(shifted(traj[a], D, recs[a]["delay_steps"], T), shifted(traj[b], D, recs[b]["delay_steps"], T), tau, discs, kw["margin"])
            assert rec["status"] in (0, 2), (a, b, rec["min_separation"])
    for i, r in enumerate(recs):
        if r["status"] < 0:
            continue
        assert r["n_tried"] == (r["delay_steps"] + 1 if r["status"] == 0 else D + 1)
        if r["n_tried"] == 1 and r["status"] == 0:
            assert r["blocker"] == -1 and r["t_block"] == 0.0 and r["s_block"] == (0.0, 0.0)
            continue
        j, d = r["blocker"], (r["delay_steps"] - 1 if r["status"] == 0 else D)
        assert 0 <= j < i and recs[j]["status"] == 0
        rec = CR.pair(shifted(traj[i], D, d, T), shifted(traj[j], D, recs[j]["delay_steps"], T), tau, discs, kw["margin"])
        assert rec["status"] == 1 and rec["t_first"] == r["t_block"] and rec["s_first"] == r["s_block"], (i, j, d)


def test_two_identical_plans_from_the_same_start_the_second_waits_or_is_blocked_for_ever():
    plans, rows = profiles()
    checked = 0
    for q in [q for q in range(N) if plans[q] is not None and plans[q].edges][:6]:
        duration = float(rows[q][-1, 2])
        for D in (int(duration / 0.1) + 5, int(duration / 0.1) + 60):
            kw = dict(t_from=0.0, t_to=2.0 * duration + 0.1 * D + 5.0, dt=0.1, margin=0.0, max_delay_steps=D)
            call = ([plans[q], plans[q]], [rows[q], rows[q]], [1.0, 1.0], [(0, 1)], POINT, LIM["a_acc"], LIM["a_dec"])
            tau, traj, recs = DR.deconflict(*call, **kw)
            first, second = recs
            assert (first["status"], first["delay_steps"], first["n_tried"], first["blocker"], first["t_start"]) == (0, 0, 1, -1, 1.0)
            d = second["delay_steps"]
            assert second["status"] == 0 and 0 < d <= int(duration / 0.1) + 1 and second["n_tried"] == d + 1 and second["blocker"] == 0
            assert second["t_start"] == 1.0 + d * 0.1 and not second["undecided"]
            check_schedule(tau, traj, recs, [(0, 1)], POINT, kw)
            # the first stands at the goal for ever: whenever the second arrives it meets it there
            _, _, held = DR.deconflict(*call, hold_after=True, **kw)
            assert (held[1]["status"], held[1]["delay_steps"], held[1]["n_tried"], held[1]["blocker"], held[1]["t_start"]) == (1, -1, D + 1, 0, 1.0)
            assert held[0]["status"] == 0 and held[1]["t_block"] > 0.0
        # starts further apart than the durations: nobody waits
        _, _, recs = DR.deconflict([plans[q], plans[q]], [rows[q], rows[q]], [1.0, 1.0 + duration + 0.35], [(0, 1)], POINT, LIM["a_acc"], LIM["a_dec"], **kw)
        assert all((r["status"], r["delay_steps"], r["n_tried"], r["blocker"]) == (0, 0, 1, -1) for r in recs)
        checked += 1
    assert checked == 6


def test_over_the_gpu_cases_no_vehicle_is_undecided_and_every_schedule_holds():
    plans, rows = profiles()
    starts = scene()[1]
    waited = blocked = without = levels = 0
    for name, (which, pairs, t_start, discs, kw) in cases(starts).items():
        tau, traj, recs = DR.deconflict([plans[q] for q in which], [rows[q] for q in which], t_start, pairs, discs, LIM["a_acc"], LIM["a_dec"], **kw)
        status = [r["status"] for r in recs]
        print("%s: %d scheduled (%d waited, longest %d), %d blocked, %d without a plan, %d levels, %d undecided" % (
            name, status.count(0), sum(r["delay_steps"] > 0 for r in recs), max(r["delay_steps"] for r in recs), status.count(1), status.count(-1),
            max(DR.levels(len(which), pairs)) + 1, sum(r["undecided"] for r in recs)))
        assert not any(r["undecided"] for r in recs), name
        check_schedule(tau, traj, recs, pairs, discs, kw)
        waited += sum(r["delay_steps"] > 0 for r in recs)
        blocked += status.count(1)
        without += status.count(-1)
        levels = max(levels, max(DR.levels(len(which), pairs)) + 1)
        if name.startswith("D=0"):
            assert all(r["delay_steps"] in (0, -1) and r["n_tried"] == 1 for r in recs if r["status"] >= 0) and status.count(1) >= 1
        if name == "chain":
            assert DR.levels(16, pairs) == list(range(16))
        if name == "star":
            assert DR.levels(16, pairs) == [0] + [1] * 15
    assert waited >= 40 and blocked >= 10 and without >= 4 and levels >= 40
