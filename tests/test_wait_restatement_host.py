"""CPU: the numpy restatement of a call with waits at stops (tests/wait_restatement.py), which tests/test_gpu_pipeline_deconflict_waits.py compares the
kernels with, run alone on the ORACLE's plans of that file's queries (the scene of tests/test_conflict_restatement_host.py) with the profiles of
tests/speed_restatement.py.  Checked without a GPU, over CASES -- the margins, starts, pair lists, lattices and place counts the GPU test uses:
 - no vehicle is undecided (no separation of a tried candidate within 1e-9 of the margin);
 - every pair of scheduled vehicles is clear on their COMPOSITE trajectories, by conflict_restatement.pair, which shares nothing with
   wait_restatement.decide;
 - a vehicle with a rejected candidate conflicts with its blocker at t_block under the last rejected candidate, first there, at the recorded arc lengths;
 - with no_start_wait set for all vehicles no place is -1 and at least one vehicle waits at a stop;
 - with max_places = 0 the decisions are delay_restatement.decide's."""
import numpy as np

import conflict_restatement as CR
import delay_restatement as DR
import wait_restatement as WR
from test_conflict_restatement_host import LIM, profiles
from test_delay_restatement_host import HOLDS, TS, cases
from test_locate_restatement_host import N, scene

DS = (0, 1, 64, 65)
PLACES = (0, 1, 4)


def wait_cases(starts):
    """the calls of the GPU test by name: (which plans, pair list or None, start times, discs, keywords of the call with max_places and no_start_wait)"""
    base = cases(starts)
    names = ["T=%d" % T for T in TS] + ["D=%d" % D for D in DS] + ["chain", "star", "all-12"] + ["nearest, " + h for h in HOLDS] + ["CAR3"]
    out = {name: base[name][:4] + (dict(base[name][4], max_places=4),) for name in names}
    which, pairs, t_start, discs, kw = base["nearest, absent"]
    for P in PLACES:
        out["max_places=%d" % P] = (which, pairs, t_start, discs, dict(kw, max_places=P))
        if P:
            out["max_places=%d, no start" % P] = (which, pairs, t_start, discs, dict(kw, max_places=P, no_start_wait=np.ones(len(which), dtype=bool)))
    which, pairs, t_start, discs, kw = base["all-12"]
    out["all-12, no start"] = (which, pairs, t_start, discs, dict(kw, max_places=4, no_start_wait=np.ones(len(which), dtype=bool)))
    return out


def restate(plans, rows, which, pairs, t_start, discs, kw, **more):
    return WR.deconflict_waits([plans[q] for q in which], [rows[q] for q in which], t_start, pairs, discs, LIM["a_acc"], LIM["a_dec"], **dict(kw, **more))


def check_schedule(tau, recs, theirs, traj, spots, pairs, discs, kw, fixed=None):
    """independent of wait_restatement.decide: every pair of scheduled vehicles is clear, and the last rejected candidate of a vehicle conflicts with
    its blocker first at t_block, at the recorded arc lengths"""
    T, D, n = len(tau), kw["max_delay_steps"], len(recs)
    for a, b in (CR.all_pairs(n) if pairs is None else pairs):
        if recs[a]["status"] == 0 and recs[b]["status"] == 0:
            rec = CR.pair(theirs[a], theirs[b], tau, discs, kw["margin"])
            assert rec["status"] in (0, 2), (a, b, rec["min_separation"])
    for i, r in enumerate(recs):
        if r["status"] < 0:
            continue
        free = fixed is None or fixed[i][0] == WR.FREE
        start = free and not (kw.get("no_start_wait") is not None and kw["no_start_wait"][i])
        tried = WR.candidates(D, start, len(spots[i])) if free else [None]
        assert r["n_tried"] == (len(tried) if r["status"] == 1 else (tried.index((r["place"], r["wait_steps"])) + 1 if free else 1)), (i, r)
        if r["status"] == 0 and r["n_tried"] == 1:
            assert r["blocker"] == -1 and r["t_block"] == 0.0 and tuple(r["s_block"]) == (0.0, 0.0)
            continue
        j = int(r["blocker"])
        assert 0 <= j < i and recs[j]["status"] in (0, 2)
        place, d = tried[r["n_tried"] - (2 if r["status"] == 0 else 1)] if free else ((WR.START if fixed[i][0] == WR.START else 0) if fixed[i][1] else WR.NO_WAIT, fixed[i][1])
        rejected = WR.composite(traj[i], place, d, T, D, spots[i][place] if place >= 0 else None)
        rec = CR.pair(rejected, theirs[j], tau, discs, kw["margin"])
        assert rec["status"] == 1 and rec["t_first"] == r["t_block"] and rec["s_first"] == tuple(r["s_block"]), (i, j, place, d)
        for k in range(j):  # (no partner of smaller index conflicts at that time or before, none at all before)
            if theirs[k] is not None and k in DR.partners_below(n, pairs)[i]:
                other = CR.pair(rejected, theirs[k], tau, discs, kw["margin"])
                assert other["status"] != 1 or other["t_first"] > r["t_block"], (i, j, k)


def test_over_the_gpu_cases_no_vehicle_is_undecided_and_every_schedule_holds():
    plans, rows = profiles()
    starts = scene()[1]
    at_start = at_stop = blocked = without = 0
    for name, (which, pairs, t_start, discs, kw) in wait_cases(starts).items():
        tau, traj, recs, undecided, theirs, spots = restate(plans, rows, which, pairs, t_start, discs, kw)
        status = list(recs["status"])
        print("%s: %d scheduled (%d wait at the start, %d at a stop, longest %d), %d blocked, %d without a plan, %d places, %d undecided" % (
            name, status.count(0), int((recs["place"] == -1).sum()), int((recs["place"] >= 0).sum()), int(recs["wait_steps"].max()), status.count(1), status.count(-1),
            sum(len(s) for s in spots if s is not None), int(undecided.sum())))
        assert not undecided.any(), name
        check_schedule(tau, recs, theirs, traj, spots, pairs, discs, kw)
        at_start += int((recs["place"] == -1).sum())
        at_stop += int((recs["place"] >= 0).sum())
        blocked += status.count(1)
        without += status.count(-1)
        if "no start" in name:
            assert not (recs["place"] == -1).any() and (recs["place"] >= 0).any(), name
        if name == "max_places=0":
            _, _, want = DR.deconflict([plans[q] for q in which], [rows[q] for q in which], t_start, pairs, discs, LIM["a_acc"], LIM["a_dec"], **{k: v for k, v in kw.items() if k != "max_places"})
            for a, b in zip(recs, want):
                assert (a["status"], a["wait_steps"], a["n_tried"], a["blocker"], a["t_start"], a["t_block"], tuple(a["s_block"])) == (
                    b["status"], b["delay_steps"], b["n_tried"], b["blocker"], b["t_start"], b["t_block"], b["s_block"])
                assert a["place"] == (-1 if b["delay_steps"] > 0 else -2) and a["row"] == -1 and a["t_hold"] == a["t_resume"] == a["s_wait"] == 0.0
    assert at_start >= 40 and at_stop >= 5 and blocked >= 10 and without >= 4


def test_a_result_fed_back_as_fixed_is_clear_and_a_fixed_wait_in_conflict_is_still_seen():
    plans, rows = profiles()
    which, pairs, t_start, discs, kw = wait_cases(scene()[1])["max_places=4, no start"]
    tau, traj, recs, undecided, theirs, spots = restate(plans, rows, which, pairs, t_start, discs, kw)
    bound = np.isin(recs["status"], (0, 2))
    fixed = np.stack([np.where(bound, np.where(recs["place"] >= 0, recs["row"], -1), -2), np.where(bound, recs["wait_steps"], 0)], axis=1)
    again = restate(plans, rows, which, pairs, t_start, discs, kw, fixed=fixed)[2]
    assert (again["status"][bound] == 0).all() and (again["blocker"][bound] == -1).all() and (again["n_tried"][bound] == 1).all()
    for name in ("t_hold", "t_resume", "s_wait", "wait_steps", "row", "t_start"):
        assert np.array_equal(again[name][bound], recs[name][bound]), name
    # a row that is no stop: -2; a vehicle that waited is held without its wait: it conflicts (2) where it was blocked, and is still seen
    waited = int(np.flatnonzero(bound & (recs["wait_steps"] > 0))[0])
    unfixed = fixed.copy()
    unfixed[waited] = (-1, 0)
    moving = next(q for q in range(waited + 1, len(which)) if bound[q] and rows[which[q]][1, 1] > 0.0)  # (below it: it changes nothing for `waited`)
    unfixed[moving] = (1, 0)
    tau, traj, other, _, theirs, spots = restate(plans, rows, which, pairs, t_start, discs, kw, fixed=unfixed)
    assert other["status"][moving] == -2 and other["wait_steps"][moving] == -1
    assert other["status"][waited] == 2 and 0 <= other["blocker"][waited] < waited and other["wait_steps"][waited] == 0 and theirs[waited] is not None
    check_schedule(tau, other, theirs, traj, spots, pairs, discs, kw, fixed=unfixed)
