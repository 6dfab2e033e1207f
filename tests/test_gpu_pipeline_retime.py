"""-m gpu: decided waits written into the timetables, by ticket (pp_pipeline_retime, pp_planner_retime; k_retime_tickets in
pathplanning_amd/csrc/pp_retime.hpp; the definition is in include/pp_hip.h).

The comparator is tests/retime_restatement.py, a restatement in numpy that shares nothing with the kernel, fed with the (s, v, t) rows that
speed_profile(samples=True) returned, so that every byte of the rows and of the records is compared, nothing within a tolerance.  The other services
are then asked about the retimed rows and compared with their own restatements fed the same rows (tests/timetable_restatement.py through
test_gpu_pipeline_timetable.compare, imported), and the loop deconflict_waits -> wait_holds -> retime -> conflicts is closed against the wait rule's
position composed in numpy from the device's own extended trajectory, within the project's pose tolerance of 1e-9.

Scene: the one of tests/test_gpu_pipeline_stamp.py (48 plans held in a capacity-64 pipeline, shared with that file when both run in one process; a
failed query among them; plans with dwelling cusp stops under V.limits(spacing=0.25, dwell=0.5)).  Every test leaves the pipeline with nothing in
flight and with a fresh speed profile: the rows a retime call wrote do not outlive the test."""
import ctypes as C

import numpy as np
import pytest

import conflict_restatement as CR
import retime_restatement as RT
import speed_restatement as V
import timetable_restatement as TT
import wait_restatement as WR
from test_gpu_pipeline_deconflict import extended_poses
from test_gpu_pipeline_stamp import CAPACITY, N, drain
from test_gpu_pipeline_timetable import compare, dwelt_plan, fleet, mixed
from test_wait_restatement_host import wait_cases

pytestmark = pytest.mark.gpu

PP_ERR_INVALID = -1
TOL = 1e-9
TWO_PI = 6.283185307179586
LIM = V.limits(spacing=0.25, dwell=0.5)
A_ACC, A_DEC = LIM["a_acc"], LIM["a_dec"]


def profile(f, which=None, **more):
    """speed_profile over the 48 tickets (or `which`): (records, rows with None for a plan without a profile)"""
    recs, rows = f.s.pipe.speed_profile(f.s.tickets if which is None else f.s.tickets[which], **dict(LIM, **more))
    return recs, [r if len(r) else None for r in rows]


def inner_stops(r):
    st = TT.stops(r, A_ACC, A_DEC)
    return st[(st["row"] > 0) & (st["row"] < len(r) - 1)]


def hold_array(entries):
    return np.array(sorted(entries), dtype=RT.HOLD_DTYPE)


def same_rows(got, want, what):
    """the rows a call returned against the restatement's, byte for byte (an empty array for a plan without a profile)"""
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        if b is None:
            assert a.shape == (0, 3), (what, i)
            continue
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a != b).any(axis=1))
            raise AssertionError((what, "plan", i, "row", int(bad[0]), a[bad[0]], b[bad[0]]))


def mixed_holds(rows, forced=()):
    """holds on a mix of plans: by the plan's index none, one at N - 1, one at every inner stop, or every inner stop and N - 1 (`forced`: these too)"""
    entries = []
    for i, r in enumerate(rows):
        if r is None:
            continue
        mode = 3 if i in forced else i % 4
        at = ([int(j) for j in inner_stops(r)["row"]] if mode >= 2 else []) + ([len(r) - 1] if mode in (1, 3) else [])
        entries += [(i, j, 0.1 + 0.37 * k + 0.01 * i) for k, j in enumerate(at)]
    return hold_array(entries)


# ------------------------------------------------------------------------------------------------------------------
def test_rows_and_records_equal_the_restatement_byte_for_byte():
    """holds on a mix of the 48 plans: none, one, two or more, one at N - 1; plans of fewer than 64 rows and of more than 128 (two passes of the wave and a
    remainder); the failed query.  Three plans are profiled from a later arc length so that a cusp stop of theirs lands on row 63, 64 and 65 of their
    window: on the scene of this file all three were reached (the test prints them, and fails if none is).  rows=True and the records equal the
    restatement applied to the rows speed_profile(samples=True) returned, byte for byte; plans without a hold keep every byte."""
    f = fleet()
    s = f.s
    recs, rows = profile(f)
    # a stop on rows 63, 64 and 65: three plans with an inner stop far enough along, their windows moved so that it lands there
    from_length, forced, free = np.full(N, -np.inf), {}, [q for q in range(N) if rows[q] is not None and len(inner_stops(rows[q]))]
    for target in (63, 64, 65):
        for q in free:
            far = [int(j) for j in inner_stops(rows[q])["row"] if j >= target]
            if far and q not in forced:
                forced[q] = target
                from_length[q] = rows[q][far[0] - target, 0]
                break
    try:
        recs, rows = profile(f, from_length=from_length)
        reached = sorted(t for q, t in forced.items() if rows[q] is not None and t < len(rows[q]) - 1 and rows[q][t, 1] == 0.0)
        print("a stop on rows", reached, "of the windows of plans", sorted(forced))
        assert reached, forced
        # ... and, whatever their index, the shortest plan and the one with the most rows behind its first inner stop get every hold they can
        shortest = min((q for q in range(N) if rows[q] is not None and q not in forced), key=lambda q: len(rows[q]))
        longest = max((q for q in free if q not in forced), key=lambda q: len(rows[q]) - int(inner_stops(rows[q])["row"][0]))
        holds = mixed_holds(rows, set(forced) | {shortest, longest})
        want_recs, want_rows = RT.retime_call(rows, holds, A_ACC, A_DEC)
        got_recs, got_rows = s.pipe.retime(s.tickets, holds, rows=True)
        assert got_recs.dtype.itemsize == 40 and got_recs.tobytes() == want_recs.tobytes(), (got_recs, want_recs)
        same_rows(got_rows, want_rows, "a mix of holds")
        solved = [q for q in range(N) if rows[q] is not None]
        per_plan = np.bincount(holds["plan"], minlength=N)
        assert len(solved) >= 40 and any(recs[q].status != 0 for q in range(N))
        assert {0, 1}.issubset(set(per_plan[solved])) and (per_plan[solved] >= 2).any() and (got_recs.status[solved] == 0).all()
        assert any(len(rows[q]) < 64 and per_plan[q] for q in solved)
        assert any(per_plan[q] >= 2 and len(rows[q]) - got_recs.first_row[q] > 128 for q in solved)  # two passes of the wave and a remainder
        assert any(per_plan[q] == 1 and got_recs.first_row[q] == len(rows[q]) - 1 for q in solved)  # a hold at N - 1 alone
        for q in solved:
            if per_plan[q] == 0:
                assert got_rows[q].tobytes() == rows[q].tobytes() and got_recs.first_row[q] == -1 and got_recs.duration[q] == got_recs.duration_before[q] == recs[q].duration
            else:
                lo = got_recs.first_row[q]
                assert got_rows[q][:lo].tobytes() == rows[q][:lo].tobytes() and got_rows[q][:, :2].tobytes() == rows[q][:, :2].tobytes()
                assert (got_rows[q][lo:, 2] > rows[q][lo:, 2]).all() and got_recs.duration[q] == got_rows[q][-1, 2] and got_recs.duration_before[q] == recs[q].duration
        for q in range(N):
            if rows[q] is None:
                assert got_recs[q].tobytes() == np.array((-1, 0, 0, -1, 0.0, 0.0, 0.0), dtype=RT.RESULT_DTYPE).tobytes()
        # no hold at all, and no rows asked for: the records alone; then the rows as they are
        again = s.pipe.retime(s.tickets, None)
        assert (again.n_holds == 0).all() and np.array_equal(again.duration[solved], got_recs.duration[solved]) and np.array_equal(again.status, np.where(got_recs.status == -1, -1, 0))
        same_rows(s.pipe.retime(s.tickets, [], rows=True)[1], want_rows, "read back")
    finally:
        profile(f)


@pytest.mark.parametrize("by", ["time", "length"])
def test_the_timetable_call_sees_the_retimed_rows(by):
    """after the call, timetable() by time and by arc length -- look-ups inside the lengthened dwells, on the held stops and around them included --
    equals timetable_restatement fed the retimed rows, by test_gpu_pipeline_timetable.compare; the stop list's t_depart is the new one"""
    f = fleet()
    s = f.s
    try:
        _, rows = profile(f)
        holds = mixed_holds(rows)
        got_recs, new = s.pipe.retime(s.tickets, holds, rows=True)
        new = [r if len(r) else None for r in new]
        same_rows([r if r is not None else np.zeros((0, 3)) for r in new], RT.retime_call(rows, holds, A_ACC, A_DEC)[1], "before the look-ups")
        values = mixed(new, by, 70, LIM, dwelt_plan(new, LIM))
        inside = 0
        for q in range(N):  # six look-ups of every plan with a held inner stop go into its lengthened dwell, onto the stop and next to it
            mine = holds[(holds["plan"] == q) & (holds["row"] < (len(rows[q]) - 1 if rows[q] is not None else 0))]
            if len(mine):
                j, w = int(mine["row"][0]), mine["seconds"][0]
                if by == "time":
                    values[q, :6] = [rows[q][j, 2], new[q][j, 2], rows[q][j, 2] + 0.5 * w, new[q][j, 2] - 1e-9, np.nextafter(new[q][j, 2], np.inf), new[q][j, 2] - 0.9 * w]
                else:
                    sj = rows[q][j, 0]
                    values[q, :6] = [sj, np.nextafter(sj, -np.inf), np.nextafter(sj, np.inf), sj - 0.01, sj + 0.01, sj]
                inside += 1
        assert inside >= 10
        got = s.pipe.timetable(s.tickets, values, by=by, max_stops=16)
        compare(got, f, range(N), new, values, by, LIM, 16, "retimed, by %s" % by)
        for q in range(N):
            if new[q] is None:
                continue
            listed = got[1][q][:got[0][q].n_listed]
            assert np.array_equal(listed.t_depart, new[q][listed.row, 2]) and got[0][q].duration == new[q][-1, 2] == got_recs.duration[q]
            for h in holds[holds["plan"] == q]:
                k = np.flatnonzero(listed.row == h["row"])
                if len(k):
                    old = TT.stops(rows[q], A_ACC, A_DEC)
                    old = old[old["row"] == h["row"]][0]
                    assert abs((listed.t_depart[k[0]] - listed.t_arrive[k[0]]) - (old["t_depart"] - old["t_arrive"] + h["seconds"])) <= 1e-12
    finally:
        profile(f)


def test_closing_the_loop_deconflict_waits_then_retime_then_conflicts():
    """deconflict_waits with every vehicle barred from its start and max_places = 4 on a 0.25 s lattice decides waits at stops; wait_holds and retime
    commit them; conflicts(poses=True) under the new starts then shows every vehicle where the wait rule's "Position under a wait" has it -- composed in
    numpy from the extended trajectory and the places downloaded BEFORE the retime -- within 1e-9 (angles mod 2 pi): the two differ only by the
    rounding of u, times v_peak.  Every listed pair of scheduled vehicles whose min_separation is further than 1e-9 from the margin is free of
    conflict, and a second deconflict_waits round with every vehicle free gives the committed vehicles no wait (place -2)."""
    from pathplanning_amd import planner
    f = fleet()
    s = f.s
    _, pairs, t_start, _, _ = wait_cases(s.starts)["nearest, absent"]
    kw = dict(t_from=0.0, t_to=40.0, dt=0.25, margin=0.5, max_delay_steps=30)
    k0, T = CR.lattice(kw["t_from"], kw["t_to"], kw["dt"])
    D = kw["max_delay_steps"]
    barred = np.ones(N, dtype=bool)
    try:
        profile(f)
        got, places, counts = s.pipe.deconflict_waits(s.tickets, t_start, pairs=pairs, no_start_wait=barred, max_places=4, places=True, **kw)
        waits = np.flatnonzero(np.isin(got.status, (0, 2)) & (got.place >= 0) & (got.wait_steps > 0))
        print("%d vehicles wait at a stop, %d are blocked, longest wait %d steps" % (len(waits), int((got.status == 1).sum()), int(got.wait_steps.max())))
        if not len(waits):
            pytest.skip("the scene decides no wait at a stop under these arguments")
        assert not (got.place == -1).any()
        before = extended_poses(s.pipe, s.tickets, t_start, kw)  # [T + D, 3] per vehicle, NaN where absent
        holds, ts = planner.wait_holds(got, kw["dt"], t_start)
        assert np.array_equal(ts, t_start) and holds["plan"].tolist() == waits.tolist() and np.array_equal(holds["row"], got.row[waits])
        assert np.array_equal(holds["seconds"], got.wait_steps[waits] * np.float64(kw["dt"]))
        recs = s.pipe.retime(s.tickets, holds)
        assert (recs.status[waits] == 0).all() and (recs.n_holds[waits] == 1).all() and np.array_equal(recs.held[waits], holds["seconds"])
        look = {k: v for k, v in kw.items() if k != "max_delay_steps"}
        traj, found, xyt = s.pipe.conflicts(s.tickets, ts, pairs=pairs, poses=True, **look)
        worst = 0.0
        for i in range(N):
            if got.status[i] == -1:
                assert traj[i].status == -1
                continue
            want = before[i][D:D + T].copy()
            if i in waits:
                spot = places[i][got.place[i]]
                assert spot.row == got.row[i]
                src = np.array([WR.source(int(c), int(spot.column), int(got.wait_steps[i])) for c in np.arange(T) + D])
                want = before[i][np.where(src < 0, 0, src)].copy()
                want[src < 0] = spot.pose
                assert (src < 0).sum() == min(got.wait_steps[i], T + D - spot.column)
            assert np.array_equal(np.isnan(want[:, 0]), np.isnan(xyt[i][:, 0])), i
            there = ~np.isnan(want[:, 0])
            err = np.abs(want[there] - xyt[i][there])
            err[:, 2] = np.abs(err[:, 2] - TWO_PI * np.rint(err[:, 2] / TWO_PI))
            assert err.max(initial=0.0) <= TOL, (i, float(err.max()))
            worst = max(worst, float(err.max(initial=0.0)))
        print("worst pose difference %.3g" % worst)
        scheduled = np.isin(got.status, (0, 2))
        checked = 0
        for (a, b), rec in zip(pairs, found):
            if scheduled[a] and scheduled[b] and got.status[a] == 0 and got.status[b] == 0 and abs(rec.min_separation - kw["margin"]) > TOL:
                assert rec.status in (0, 2), (a, b, rec.status, rec.min_separation)
                checked += 1
        assert checked >= 20  # (not vacuous: with the starts barred many vehicles find no clear candidate, and their pairs do not count)
        again = s.pipe.deconflict_waits(s.tickets, ts, pairs=pairs, no_start_wait=barred, max_places=4, **kw)
        assert (again.place[waits] == -2).all() and (again.status[waits] == 0).all() and (again.wait_steps[waits] == 0).all(), again[waits]
    finally:
        profile(f)


def test_a_hold_on_a_moving_row_one_beyond_the_dwell_and_a_plan_without_a_profile():
    """-2 for a hold on a moving row, -3 with the right bad_hold for a negative hold larger than the dwell (behind a valid hold of the same plan), -1 for
    the failed query, whose holds are skipped; in each case the plan's rows keep every byte, and the other plans of the same call are applied"""
    f = fleet()
    s = f.s
    try:
        recs, rows = profile(f)
        failed = next(q for q in range(N) if rows[q] is None)
        dwelt = [q for q in range(N) if rows[q] is not None and any(d > 0.4 for d in (lambda st: st["t_depart"] - st["t_arrive"])(inner_stops(rows[q])))]
        assert len(dwelt) >= 3
        a, b, c = dwelt[0], dwelt[1], dwelt[2]
        moving = int(np.flatnonzero(rows[a][:, 1] > 0.0)[len(rows[a]) // 3])
        st = inner_stops(rows[b])
        cusp = int(st["row"][np.flatnonzero(st["t_depart"] - st["t_arrive"] > 0.4)[-1]])
        earlier = [int(j) for j in TT.stops(rows[b], A_ACC, A_DEC)["row"] if 0 < j < cusp]
        st_c = inner_stops(rows[c])
        cusp_c = int(st_c["row"][np.flatnonzero(st_c["t_depart"] - st_c["t_arrive"] > 0.4)[0]])
        entries = [(a, moving, 1.0), (a, len(rows[a]) - 1, 1.0), (b, cusp, -0.75), (b, len(rows[b]) - 1, 5.0), (c, cusp_c, -0.25),
                   (c, len(rows[c]) - 1, 0.5), (failed, 5, 1.0), (failed, 7, -100.0)] + [(b, j, 0.5) for j in earlier[:1]]
        holds = hold_array(entries)
        want_recs, want_rows = RT.retime_call(rows, holds, A_ACC, A_DEC)
        got_recs, got_rows = s.pipe.retime(s.tickets, holds, rows=True)
        assert got_recs.tobytes() == want_recs.tobytes(), (got_recs[[a, b, c, failed]], want_recs[[a, b, c, failed]])
        same_rows(got_rows, want_rows, "statuses")
        assert (got_recs.status[a], got_recs.status[b], got_recs.status[c], got_recs.status[failed]) == (-2, -3, 0, -1)
        assert holds[got_recs.bad_hold[a]].tolist() == (a, moving, 1.0) and holds[got_recs.bad_hold[b]].tolist() == (b, cusp, -0.75) and got_recs.bad_hold[c] == -1
        assert got_recs.bad_hold[failed] == -1 and got_recs.n_holds[failed] == 0 and got_recs.n_holds[a] == 2 and got_recs.n_holds[b] == 2 + len(earlier[:1])
        assert got_rows[a].tobytes() == rows[a].tobytes() and got_rows[b].tobytes() == rows[b].tobytes() and got_rows[c].tobytes() != rows[c].tobytes()
        assert abs((got_recs.duration[c] - got_recs.duration_before[c]) - 0.25) <= 1e-12 and got_recs.held[a] == got_recs.held[b] == 0.0
        # exactly the dwell is still valid: delta + w == 0
        delta = RT.dwell(got_rows[b], cusp, A_ACC, A_DEC)
        one = s.pipe.retime(s.tickets[[b]], [(0, cusp, -delta)], rows=True)
        assert one[0].status[0] == 0 and RT.dwell(one[1][0], cusp, A_ACC, A_DEC) == 0.0
        below = s.pipe.retime(s.tickets[[b]], [(0, cusp, np.nextafter(0.0, -1.0))])
        assert below[0].status in (0, -3)  # (a dwell of zero to one ulp: either side of the rule, by the restatement below)
        assert below[0].status == RT.retime(one[1][0], [(cusp, np.nextafter(0.0, -1.0))], A_ACC, A_DEC)[0]["status"]
    finally:
        profile(f)


def test_two_calls_accumulate_and_a_new_speed_profile_call_resets():
    """two calls of w give the bytes of the restatement applied twice; -w afterwards restores the times to rounding; a new speed_profile call restores
    the original rows bit for bit"""
    f = fleet()
    s = f.s
    try:
        _, rows = profile(f)
        holds = mixed_holds(rows)
        _, once = RT.retime_call(rows, holds, A_ACC, A_DEC)
        want_recs, twice = RT.retime_call(once, holds, A_ACC, A_DEC)
        s.pipe.retime(s.tickets, holds)
        got_recs, got_rows = s.pipe.retime(s.tickets, holds, rows=True)
        assert got_recs.tobytes() == want_recs.tobytes()
        same_rows(got_rows, twice, "two calls")
        # -w after +w, at the cusp stops that dwell 0.5 s (where the speed profile left no dwell, -w may miss the rule by one ulp: status -3, as defined)
        _, fresh = profile(f)
        entries = []
        for q in range(N):
            if rows[q] is not None:
                st = inner_stops(rows[q])
                entries += [(q, int(j), 0.3 + 0.01 * q) for j in st["row"][st["t_depart"] - st["t_arrive"] > 0.4]]
        there = hold_array(entries)
        back = there.copy()
        back["seconds"] = -there["seconds"]
        assert len(there) >= 10
        s.pipe.retime(s.tickets, there)
        recs, restored = s.pipe.retime(s.tickets, back, rows=True)
        same_rows(restored, RT.retime_call(RT.retime_call(rows, there, A_ACC, A_DEC)[1], back, A_ACC, A_DEC)[1], "there and back")
        for q in range(N):
            if rows[q] is not None:
                assert recs.status[q] == 0 and np.abs(restored[q] - rows[q]).max() <= 1e-9 and restored[q][:, :2].tobytes() == rows[q][:, :2].tobytes()
        _, fresh = profile(f)
        same_rows([r if r is not None else np.zeros((0, 3)) for r in fresh], rows, "a new speed profile")
        same_rows(s.pipe.retime(s.tickets, None, rows=True)[1], rows, "read back after the new speed profile")
    finally:
        profile(f)


def test_refusals_launch_nothing_write_nothing_and_leave_the_pipeline_usable():
    """every refusal is PP_ERR_INVALID with the first offender named; after each, the rows fetched with retime(tickets, [], rows=True) are the rows of
    before, byte for byte; at the end the pipeline still plans"""
    from pathplanning_amd._lib import PPError, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    try:
        recs, rows = pipe.speed_profile(held[:8], **LIM)
        assert recs[0].status == 0 and recs[1].status == 0
        first = pipe.retime(held[:8], [], rows=True)
        n0 = recs[0].n_samples
        stop0 = int(inner_stops(rows[0])["row"][0]) if len(inner_stops(rows[0])) else n0 - 1
        out = np.zeros(128, dtype=RT.RESULT_DTYPE)

        def refused(tickets, entries, *words, n=None, n_holds=None, null=False):
            t = np.ascontiguousarray(tickets, dtype=np.uint64)
            hd = np.array(entries, dtype=RT.HOLD_DTYPE)
            rc = lib.pp_pipeline_retime(pipe.h, len(t) if n is None else n, ptr(t), len(hd) if n_holds is None else n_holds, None if null or not len(hd) else ptr(hd), None, ptr(out))
            msg = lib.pp_last_error().decode()
            print(rc, msg)
            assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)
            now = pipe.retime(held[:8], [], rows=True)
            assert now[0].tobytes() == first[0].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(now[1], first[1])), msg

        good = [(0, stop0, 1.0)]
        refused((held + held)[:CAPACITY + 1], good, "capacity")
        refused(held[:1], good, "capacity", n=-1)
        refused([held[0], 10 ** 9], good, "ticket %d" % 10 ** 9, "unknown")
        refused([held[3], held[4], held[3]], good, "ticket %d" % held[3], "twice")
        refused([held[0], held[9]], good, "ticket %d" % held[9], "speed_profile first")  # held, but not in the last speed-profile call
        refused(held[:2], good, "n_holds", n_holds=-1)
        refused(held[:2], good, "null holds", null=True)
        for plan in (-1, 2):
            refused(held[:2], [(plan, 1, 1.0)], "plan %d" % plan)
        refused(held[:2], [(0, 0, 1.0)], "ticket %d" % held[0], "row 0", "t_start")
        refused(held[:2], [(1, -3, 1.0)], "ticket %d" % held[1], "row -3")
        refused(held[:2], [(0, n0, 1.0)], "ticket %d" % held[0], "row %d" % n0, "%d rows" % n0)
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused(held[:2], good + [(1, recs[1].n_samples - 1, bad)], "ticket %d" % held[1], "not finite")
        refused(held[:2], [(0, stop0, 1.0), (0, stop0, 1.0)], "ascending", "hold 1")
        refused(held[:2], [(0, n0 - 1, 1.0), (0, stop0, 1.0)] if stop0 < n0 - 1 else [(0, 2, 1.0), (0, 1, 1.0)], "ascending", "hold 1")
        refused(held[:2], [(1, 1, 1.0), (0, 1, 1.0)], "ascending", "hold 1")
        refused(held[:2], [(0, j, 0.0) for j in range(1, (1 << 10) + 2)], "ticket %d" % held[0], "more than 1024 holds")
        # the batch entry on the pipeline's buffer set
        rc = lib.pp_planner_retime(pipe.planner_h, 1, 0, None, None, ptr(out))
        assert rc == PP_ERR_INVALID and "pp_pipeline_retime" in lib.pp_last_error().decode()
        # a query in flight: its ticket is refused; held but never profiled: refused; released: refused
        flying = pipe.submit(s.goals[8:9], s.starts[8:9], np.array([955], dtype=np.uint64))
        assert len(flying) == 1 and pipe.in_flight() == 1
        refused([held[0], int(flying[0])], good, "ticket %d" % int(flying[0]), "in flight")
        res = drain(pipe, 1)
        assert res[int(flying[0])].status == 0  # the pipeline still plans
        refused([held[0], int(flying[0])], good, "ticket %d" % int(flying[0]), "speed_profile first")
        pipe.release(flying)
        refused([held[0], int(flying[0])], good, "ticket %d" % int(flying[0]), "released")
        with pytest.raises(PPError) as e:
            pipe.retime(held[:2], [(0, 0, 1.0)])
        assert e.value.code == PP_ERR_INVALID and "t_start" in str(e.value)
        with pytest.raises(ValueError):
            pipe.retime(held[:2], [(0, 1.5, 1.0)])
        # n == 0 is PP_OK; and the call of before still works and is applied
        assert lib.pp_pipeline_retime(pipe.h, 0, None, 0, None, None, None) == 0
        assert pipe.retime([], None).shape == (0,)
        done = pipe.retime(held[:8], good, rows=True)
        want = RT.retime_call([r if len(r) else None for r in rows], hold_array(good), A_ACC, A_DEC)
        assert done[0].tobytes() == want[0].tobytes()
        same_rows(done[1], want[1], "after the refusals")
    finally:
        profile(f)


def test_beside_queries_in_flight_the_buffers_grow_and_the_batch_form_gives_the_same_bytes():
    """a call with more plans and more holds than any before it, beside eight queries in flight: every buffer of the service grows, the outgrown ones are
    parked, and rows and records are the restatement's; HybridAStarBatch.retime on the same queries gives the pipeline's bytes"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError
    f = fleet()
    s = f.s
    try:
        recs, rows = s.pipe.speed_profile(s.all_tickets, **LIM)
        rows = [r if len(r) else None for r in rows]
        small = hold_array([(0, len(rows[0]) - 1, 0.5)]) if rows[0] is not None else hold_array([])
        s.pipe.retime(s.all_tickets[:1], small)
        _, rows_now = RT.retime_call(rows[:1], small, A_ACC, A_DEC)
        rows_now = rows_now + rows[1:]
        flying = s.pipe.submit(s.goals[8:16], s.starts[8:16], np.arange(960, 968, dtype=np.uint64))
        assert len(flying) == 8 and s.pipe.in_flight() == 8
        entries = []
        for i, r in enumerate(rows_now):
            if r is not None:
                entries += [(i, int(j), 0.25 + 0.01 * i) for j in TT.stops(r, A_ACC, A_DEC)["row"] if j > 0]
        holds = hold_array(entries)
        got_recs, got_rows = s.pipe.retime(s.all_tickets, holds, rows=True)
        assert s.pipe.in_flight() == 8
        drain(s.pipe, 8)
        s.pipe.release(flying)
        want_recs, want_rows = RT.retime_call(rows_now, holds, A_ACC, A_DEC)
        assert got_recs.tobytes() == want_recs.tobytes() and len(got_recs) == N + 2 and len(holds) > N
        same_rows(got_rows, want_rows, "beside queries in flight")
        same_rows(s.pipe.retime(s.all_tickets, None, rows=True)[1], want_rows, "idle, read back")
        # the batch form
        n = 16
        batch = pa.HybridAStarBatch(s.val, max_batch=n, max_nodes=32768)
        batch.initialize(s.pipe.nonholo_table())
        res = batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
        assert sum(r.status == 0 for r in res) >= 4
        with pytest.raises(PPError) as e:
            batch.retime(None)
        assert e.value.code == PP_ERR_INVALID and "query 0" in str(e.value) and "speed_profile first" in str(e.value)
        lim = V.limits(spacing=0.2, dwell=1.0)
        _, mine = batch.speed_profile(**lim)
        _, theirs = s.pipe.speed_profile(s.tickets[:n], **lim)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(mine, theirs))
        holds = mixed_holds([r if len(r) else None for r in mine], forced=(2, 6))
        a, b = batch.retime(holds, rows=True), s.pipe.retime(s.tickets[:n], holds, rows=True)
        assert a[0].tobytes() == b[0].tobytes() and (a[0].n_holds > 0).sum() >= 3
        same_rows(a[1], [r if len(r) else None for r in b[1]], "batch form")
        same_rows(a[1], RT.retime_call([r if len(r) else None for r in mine], holds, lim["a_acc"], lim["a_dec"])[1], "batch form against the restatement")
        some = batch.retime(None, n_queries=5, rows=True)
        assert len(some[0]) == 5 and all(x.tobytes() == y.tobytes() for x, y in zip(some[1], a[1][:5]))
        batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
        with pytest.raises(PPError) as e:
            batch.retime(None)
        assert "speed_profile first" in str(e.value)
        batch.close()
    finally:
        profile(f)
