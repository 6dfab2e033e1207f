"""CPU: the numpy restatement of a retime call (tests/retime_restatement.py), which tests/test_gpu_pipeline_retime.py compares the kernel with, run
alone on the ORACLE's plans (the scene of tests/test_conflict_restatement_host.py) with the profiles of tests/speed_restatement.py.  Checked without a
GPU:
 - timetable_restatement.stops of the retimed rows shows t_depart - t_arrive grown by the hold, to 1e-12, at the held stop and nowhere else, and every
   stop behind it arrives later by the holds at or before it;
 - the wait rule's position (wait_restatement: the composite trajectory of a wait of d steps at a stop's row) equals conflict_restatement's position
   on the rows retimed by the hold (row, d * dt), within 1e-9 m at every column of a 0.25 s lattice: what include/pp_hip.h states as the call's
   consequence.  The two differ only by the rounding of u, times the speed."""
import numpy as np

import conflict_restatement as CR
import retime_restatement as RT
import timetable_restatement as TT
import wait_restatement as WR
from test_conflict_restatement_host import LIM, profiles

A_ACC, A_DEC = LIM["a_acc"], LIM["a_dec"]


def inner_stops(rows):
    st = TT.stops(rows, A_ACC, A_DEC)
    return st[(st["row"] > 0) & (st["row"] < len(rows) - 1)]


def test_the_stops_of_the_retimed_rows_stand_longer_by_the_hold():
    plans, rows = profiles()
    held = dwelt = 0
    for q, r in enumerate(rows):
        if r is None:
            continue
        before = TT.stops(r, A_ACC, A_DEC)
        inner = inner_stops(r)
        # one hold at every inner stop and one at N - 1; then one hold alone, which also shortens a dwell again
        holds = [(int(j), 0.3 + 0.11 * k) for k, j in enumerate(inner["row"])] + [(len(r) - 1, 2.0)]
        rec, new = RT.retime(r, holds, A_ACC, A_DEC)
        assert rec["status"] == 0 and rec["n_holds"] == len(holds) and rec["first_row"] == holds[0][0], q
        assert new[:, :2].tobytes() == r[:, :2].tobytes() and new[:holds[0][0]].tobytes() == r[:holds[0][0]].tobytes(), q
        after = TT.stops(new, A_ACC, A_DEC)
        assert np.array_equal(after["row"], before["row"]) and np.array_equal(after["s"], before["s"])
        grown = (after["t_depart"] - after["t_arrive"]) - (before["t_depart"] - before["t_arrive"])
        want = np.array([dict(holds).get(int(j), 0.0) for j in before["row"]])
        assert np.abs(grown - want).max() <= 1e-12, (q, grown, want)
        total = np.array([sum(w for j, w in holds if j < row) for row in before["row"]])  # the holds strictly before a stop delay its arrival
        assert np.abs((after["t_arrive"] - before["t_arrive"]) - total).max() <= 1e-12, q
        assert abs(rec["held"] - sum(w for _, w in holds)) <= 1e-12 and abs((rec["duration"] - rec["duration_before"]) - rec["held"]) <= 1e-12
        held += len(holds)
        for j, d0 in zip(inner["row"], inner["t_depart"] - inner["t_arrive"]):
            if d0 > 0.4:  # a cusp stop that dwells 0.5 s: a negative hold within the dwell is applied, one beyond it is refused whole
                rec, new = RT.retime(r, [(int(j), -0.25)], A_ACC, A_DEC)
                st = TT.stops(new, A_ACC, A_DEC)
                k = int(np.flatnonzero(st["row"] == j)[0])
                assert rec["status"] == 0 and abs((st["t_depart"][k] - st["t_arrive"][k]) - (d0 - 0.25)) <= 1e-12
                rec, new = RT.retime(r, [(int(j), -0.75), (len(r) - 1, 1.0)], A_ACC, A_DEC, first=3)
                assert rec["status"] == -3 and rec["bad_hold"] == 3 and new.tobytes() == r.tobytes()
                dwelt += 1
        moving = np.flatnonzero(r[:, 1] > 0.0)
        if len(moving):
            rec, new = RT.retime(r, [(int(moving[0]), 1.0)], A_ACC, A_DEC)
            assert rec["status"] == -2 and rec["bad_hold"] == 0 and new.tobytes() == r.tobytes()
    print("%d holds on %d plans, %d dwelling cusp stops" % (held, sum(r is not None for r in rows), dwelt))
    assert held >= 60 and dwelt >= 10


def test_the_wait_rules_position_is_the_position_on_the_retimed_rows():
    plans, rows = profiles()
    dt, k0 = 0.25, 0
    compared, worst = 0, 0.0
    for q, (p, r) in enumerate(zip(plans, rows)):
        if r is None or not len(inner_stops(r)):
            continue
        t0 = 0.0123 + 0.37 * (q % 5)
        for d in (1, 3, 8):
            T = int((t0 + r[-1, 2] + d * dt) / dt) + 4
            tau = CR.times(k0, T, dt)
            traj = CR.trajectory(p, r, t0, tau, A_ACC, A_DEC, True, True)
            every = WR.stop_places(p, r, t0, k0, T, dt, A_ACC, A_DEC)
            for spot in every[(every["row"] > 0) & (every["row"] < len(r) - 1)]:
                assert spot["column"] < T
                under_wait = WR.composite(traj, 0, d, T, 0, spot)
                rec, new = RT.retime(r, [(int(spot["row"]), np.float64(d) * np.float64(dt))], A_ACC, A_DEC)
                assert rec["status"] == 0
                present, s = CR.position(new, tau - np.float64(t0), A_ACC, A_DEC, True, True)
                assert present.all() and under_wait["present"].all()
                assert under_wait["standing"].sum() == d and (s[under_wait["standing"]] == spot["s"]).all(), (q, d, spot["row"])
                err = np.abs(under_wait["s"] - s).max()
                assert err <= 1e-9, (q, d, int(spot["row"]), err)
                worst = max(worst, err)
                compared += T
    print("%d columns compared, worst |s| difference %.3g m" % (compared, worst))
    assert compared > 5000
