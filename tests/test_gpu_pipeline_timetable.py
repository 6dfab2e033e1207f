"""-m gpu: timetable look-ups and stops, by ticket (pp_pipeline_timetable, pp_planner_timetable; k_timetable_tickets in
pathplanning_amd/csrc/pp_timetable.hpp; the definition is in include/pp_hip.h).

The comparator is tests/timetable_restatement.py, a restatement in numpy that shares nothing with the kernel, fed with the (s, v, t) rows that
speed_profile(samples=True) returned, so that everything taken from the rows is bit-exact; the plans' edges are rebuilt from get_path_of as
tests/test_gpu_pipeline_locate.py rebuilds them.  EQUAL bit for bit: status, row, s, t, v, a, t_remaining, next_stop, s_to_stop, t_to_stop, the plan
records and the whole stop list.  Pose and kappa agree within 1e-9.  Edge, direction and ratio (within 1e-9) are compared for DECIDED look-ups: the arc
length more than 1e-9 from every junction S_e and no closer than speed_restatement.GUARD to a boundary between two Reeds-Shepp motions.  At most
footprint_ref.MAX_LEFT_OUT of the fleet's look-ups may be undecided (tests/test_timetable_restatement_host.py checks on the CPU that the
restatement alone stays within that on the oracle's plans, with the same choice of values).  The cap is asserted where the values are chosen that way: the
fleet's 70 look-ups per plan.  The tests that put look-ups into every dwell on purpose -- a cusp stop at a junction of two edges is undecided by nature --
compare the same fields under the same rule and do not count.

Scene: the one of tests/test_gpu_pipeline_stamp.py (48 plans held in a capacity-64 pipeline, shared with that file when both run in one process); it
has a failed query and no one-pose plan (tests/cpp/test_pipeline_timetable.cpp has one).  Every test leaves the pipeline without a footprint and with
nothing in flight."""
import ctypes as C
import functools

import numpy as np
import pytest

import conflict_restatement as CR
import footprint_ref as FR
import speed_restatement as V
import timetable_restatement as TT
from test_conflict_restatement_host import starts_of
from test_gpu_pipeline_locate import restated
from test_gpu_pipeline_stamp import CAPACITY, N, drain, scene

pytestmark = pytest.mark.gpu

PP_ERR_INVALID = -1
TOL = 1e-9
TWO_PI = 6.283185307179586
LIM = V.limits(spacing=0.25, dwell=0.5)
EXACT = ("status", "row", "s", "t", "v", "a", "t_remaining", "next_stop", "s_to_stop", "t_to_stop", "reserved", "reserved1")


class Fleet:
    def __init__(self):
        self.s = scene()
        self.plans = restated(self.s.P)  # all N + 2


@functools.lru_cache(maxsize=None)
def fleet():
    return Fleet()


def profile(f, lim=LIM, which=None):
    """speed_profile over the 48 tickets (or `which`): (records, rows with None for a plan without a profile)"""
    recs, rows = f.s.pipe.speed_profile(f.s.tickets if which is None else f.s.tickets[which], **lim)
    return recs, [r if len(r) else None for r in rows]


def dwelt_plan(rows, lim):
    """the first plan with a cusp stop that dwells (as tests/test_timetable_restatement_host.py chooses it): its look-ups include its stops and dwells"""
    for q, r in enumerate(rows):
        if r is not None:
            st = TT.stops(r, lim["a_acc"], lim["a_dec"])
            if (st["t_arrive"] < st["t_depart"]).any():
                return q
    raise AssertionError("the scene has no cusp stop")


def compare(got, f, which, rows, values, by, lim, max_stops, what):
    """the three record arrays of the device against the restatement's, plan by plan; returns (look-ups, undecided look-ups)"""
    plans, stops, out = got
    assert plans.shape == (len(which),) and stops.shape == (len(which), max_stops) and out.shape == (len(which), values.shape[1]), what
    looked = undecided = 0
    for i, q in enumerate(which):
        rec, listed, want, decided = TT.timetable(f.plans[q] if rows[i] is not None else None, rows[i], values[i], by, lim["a_acc"], lim["a_dec"], max_stops)
        here = (what, "plan", q)
        assert plans[i].tobytes() == rec.tobytes(), here + (plans[i], rec)
        padded = np.zeros(max_stops, dtype=TT.STOP_DTYPE)
        padded[:len(listed)] = listed
        assert stops[i].tobytes() == padded.tobytes(), here + ("stops", stops[i][:len(listed) + 1], listed)
        g = out[i]
        for name in EXACT:
            a, b = np.ascontiguousarray(g[name]), np.ascontiguousarray(want[name])
            if a.tobytes() != b.tobytes():
                bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))
                raise AssertionError(here + (name, "look-up", int(bad[0]), float(values[i][bad[0]]), a[bad[0]], b[bad[0]]))
        if rec["status"] < 0:
            assert g.tobytes() == want.tobytes(), here  # (status -1 and zero bytes elsewhere)
            continue
        err = np.abs(g["pose"] - want["pose"])
        err[:, 2] = np.abs(err[:, 2] - TWO_PI * np.rint(err[:, 2] / TWO_PI))
        assert err.max(initial=0.0) <= TOL, here + ("pose", float(err.max()))
        assert np.abs(g["kappa"] - want["kappa"]).max(initial=0.0) <= TOL, here + ("kappa",)
        k = np.flatnonzero(decided)
        assert np.array_equal(g["edge"][k], want["edge"][k]) and np.array_equal(g["direction"][k], want["direction"][k]), here + ("edge / direction",)
        assert np.abs(g["ratio"][k] - want["ratio"][k]).max(initial=0.0) <= TOL, here + ("ratio",)
        looked += len(decided)
        undecided += int((~decided).sum())
    print("%s: %d plans, %d look-ups, %d undecided" % (what, len(which), looked, undecided))
    return looked, undecided


def mixed(rows, by, P, lim, dwelt=None):
    return np.array([TT.mixed_values(r, by, P, lim["a_acc"], lim["a_dec"], seed=q, stops_too=q == dwelt) for q, r in enumerate(rows)]).reshape(len(rows), P)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["length", "time"])
def test_seventy_look_ups_per_plan_of_the_fleet(by):
    """all 48 plans (a failed query among them; plans with a junction cusp and a dwell; plans whose Reeds-Shepp edge reverses inside), P = 70: two passes
    of the lane loop and a remainder.  Values before, behind and inside the profile, exactly on rows and -- for one plan -- on its stops and inside its
    dwells"""
    f = fleet()
    s = f.s
    recs, rows = profile(f)
    values = mixed(rows, by, 70, LIM, dwelt_plan(rows, LIM))
    got = s.pipe.timetable(s.tickets, values, by=by)
    looked, undecided = compare(got, f, range(N), rows, values, by, LIM, 16, "by %s" % by)
    failed = [q for q in range(N) if recs[q].status != 0]
    assert failed and all(got[0][q].status == -1 and (got[2][q].status == -1).all() for q in failed)
    solved = [q for q in range(N) if recs[q].status == 0]
    assert len(solved) >= 40 and looked == 70 * len(solved) and undecided <= FR.MAX_LEFT_OUT * looked
    for q in solved:
        assert set(np.unique(got[2][q].status)) == {0, 1, 2} and got[0][q].n_stops >= 2 and got[0][q].duration == recs[q].duration
        assert got[0][q].n_samples == recs[q].n_samples and got[0][q].s_first == recs[q].s_first and got[0][q].s_last == recs[q].s_last
    assert any(got[0][q].n_stops > 2 for q in solved)  # a cusp stop
    # the same call again: the same bytes (no atomic, no order of arrival)
    again = s.pipe.timetable(s.tickets, values, by=by)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_the_arc_length_by_time_is_the_conflict_calls_trajectory():
    """timetable(by="time", tau - t_start) against conflicts(poses=True) over the same lattice and starts: present exactly where the status is 0, the same
    poses, and the plan record's s_enter / s_leave are the look-ups' s at the first and the last time present, bit for bit"""
    f = fleet()
    s = f.s
    recs, rows = profile(f)
    t_start = starts_of(N)
    kw = dict(t_from=0.0, t_to=12.95, dt=0.1)
    tau = CR.times(*CR.lattice(kw["t_from"], kw["t_to"], kw["dt"]), kw["dt"])
    traj, _, xyt = s.pipe.conflicts(s.tickets, t_start, poses=True, **kw)
    values = tau[None, :] - t_start[:, None]
    plans, _, out = s.pipe.timetable(s.tickets, values, by="time", max_stops=0)
    checked = 0
    for q in range(N):
        if recs[q].status != 0:
            assert traj[q].status == -1 and plans[q].status == -1
            continue
        present = ~np.isnan(xyt[q][:, 0])
        assert np.array_equal(out[q].status == 0, present) and np.array_equal(out[q].status == 1, values[q] < 0.0), q
        assert np.abs(out[q].pose[present] - xyt[q][present]).max(initial=0.0) <= TOL, q
        if present.any():
            k = np.flatnonzero(present)
            assert (traj[q].first, traj[q].last) == (k[0], k[-1])
            assert np.float64(traj[q].s_enter).tobytes() == out[q].s[k[0]].tobytes() and np.float64(traj[q].s_leave).tobytes() == out[q].s[k[-1]].tobytes(), q
            checked += 1
        assert (out[q].next_stop == -1).all() and plans[q].n_listed == 0 and plans[q].n_stops >= 2
    assert checked >= 40
    compare((plans, np.zeros((N, 0), dtype=TT.STOP_DTYPE), out), f, range(N), rows, values, "time", LIM, 0, "the conflict call's lattice")


def test_locate_then_timetable_then_conflicts_re_anchored():
    """the loop the call is for: a vehicle stands on its plan at a chosen arc length; locate finds s; timetable(by="length") gives the time t the
    timetable has it there; conflicts with t_start = now - t shows the vehicle at that arc length at the lattice time nearest `now`, within v_peak * dt"""
    f = fleet()
    s = f.s
    recs, rows = profile(f)
    which = [q for q in range(N) if recs[q].status == 0 and recs[q].s_last > 8.0][:12]
    assert len(which) == 12
    chosen = np.array([0.31 + 0.47 * recs[q].s_last for q in which])  # somewhere in the middle of each plan
    tickets = s.tickets[which]
    on_plan = s.pipe.timetable(tickets, chosen[:, None], by="length", max_stops=0)[2][:, 0]
    located = s.pipe.locate(tickets, on_plan.pose, spacing=LIM["spacing"])
    s_located = np.array([r.s for r in located])
    assert all(r.status == 0 and r.distance <= LIM["spacing"] / 32 for r in located)  # (on the plan, at the chosen point or where the plan passes it again)
    at = s.pipe.timetable(tickets, s_located[:, None], by="length", max_stops=0)[2][:, 0]
    assert (at.status == 0).all() and (at.t > 0.0).all() and np.array_equal(at.s, s_located)
    now, dt = 1234.567, 0.1
    t_start = now - at.t
    nearest = round(now / dt) * dt
    traj = s.pipe.conflicts(tickets, t_start, t_from=nearest - dt / 4, t_to=nearest + dt / 4, dt=dt)[0]
    for i, q in enumerate(which):
        assert traj[i].status == 0 and traj[i].n_present == 1
        assert abs(traj[i].s_enter - s_located[i]) <= recs[q].v_peak * dt, (q, traj[i].s_enter, s_located[i])
    # the set-point at the located arc length is the profile's
    for i, q in enumerate(which):
        assert 0.0 <= at.v[i] <= recs[q].v_peak + TOL and 0.0 <= at.t_remaining[i] <= recs[q].duration and abs(at.a[i]) <= LIM["a_dec"] * (1.0 + TOL)


def test_stops_dwells_that_the_lattice_step_does_not_divide_and_lists_cut_short():
    """dwell 0.37 s and look-ups every 0.1 s: the times inside a dwell stand on the stop (v = a = 0, the stop's s), the stop is the next one until the
    vehicle has left it; max_stops of 0, 1 and more than any plan has; the failed query is -1 with zero bytes; rows of stops_host behind n_listed stay"""
    from pathplanning_amd._lib import TimetableParams, ptr
    f = fleet()
    s = f.s
    lim = V.limits(spacing=0.25, dwell=0.37)
    recs, rows = profile(f, lim)
    T = 1 + int(max(r.duration for r in recs) / 0.1) + 3
    values = np.broadcast_to(-0.1 + 0.1 * np.arange(T), (N, T)).copy()
    most = 0
    for max_stops in (0, 1, 40):
        got = s.pipe.timetable(s.tickets, values, by="time", max_stops=max_stops)
        compare(got, f, range(N), rows, values, "time", lim, max_stops, "dwell 0.37, max_stops %d" % max_stops)
        most = max(most, int(got[0].n_stops.max()))
        assert (got[0].n_listed == np.minimum(got[0].n_stops, max_stops)).all()
    assert 2 < most < 40
    plans, stops, out = got
    dwelt = 0
    for q in range(N):
        if recs[q].status != 0:
            assert plans[q].status == -1 and plans[q].tobytes()[4:] == bytes(36) and (out[q].status == -1).all() and not stops[q].tobytes().strip(b"\0")
            assert all(o.tobytes()[4:] == bytes(124) for o in out[q])
            continue
        for k in range(1, plans[q].n_listed - 1):
            st = stops[q][k]
            if not st.t_arrive < st.t_depart:
                continue
            assert abs((st.t_depart - st.t_arrive) - 0.37) < 1e-12
            inside = np.flatnonzero((values[q] >= st.t_arrive) & (values[q] < st.t_depart))
            assert 3 <= len(inside) <= 4
            assert (out[q].s[inside] == st.s).all() and (out[q].v[inside] == 0.0).all() and (out[q].a[inside] == 0.0).all()
            assert (out[q].row[inside] == st.row - 1).all() and (out[q].next_stop[inside] == k).all() and (out[q].s_to_stop[inside] == 0.0).all()
            assert (out[q].t_to_stop[inside] <= 0.0).all()  # (it has arrived)
            dwelt += 1
    assert dwelt >= 1
    # through the C ABI: a pre-filled stops_host keeps its rows behind n_listed; NULL stops_host still counts and lists (next_stop refers to the list)
    t = np.ascontiguousarray(s.tickets, dtype=np.uint64)
    tp = TimetableParams(1, 40)
    mine = np.full((N, 40), 0x5A, dtype=np.uint8).repeat(32, axis=1).view(TT.STOP_DTYPE).reshape(N, 40)
    recs_c, out_c = np.zeros(N, dtype=TT.PLAN_DTYPE), np.zeros((N, T), dtype=TT.RESULT_DTYPE)
    assert s.pipe.lib.pp_pipeline_timetable(s.pipe.h, N, ptr(t), T, ptr(values), C.byref(tp), ptr(recs_c), ptr(mine), ptr(out_c)) == 0
    assert recs_c.tobytes() == plans.tobytes() and out_c.tobytes() == out.tobytes()
    for q in range(N):
        n = int(recs_c[q]["n_listed"])
        assert mine[q, :n].tobytes() == stops[q, :n].tobytes() and mine[q, n:].tobytes() == bytes([0x5A]) * (32 * (40 - n)), q
    for mask in range(7):
        a, b, c = mask & 1, mask & 2, mask & 4
        p2, s2, o2 = np.zeros(N, dtype=TT.PLAN_DTYPE), np.zeros((N, 40), dtype=TT.STOP_DTYPE), np.zeros((N, T), dtype=TT.RESULT_DTYPE)
        assert s.pipe.lib.pp_pipeline_timetable(s.pipe.h, N, ptr(t), T, ptr(values), C.byref(tp), ptr(p2) if a else None, ptr(s2) if b else None, ptr(o2) if c else None) == 0
        assert (not a or p2.tobytes() == plans.tobytes()) and (not b or s2.tobytes() == stops.tobytes()) and (not c or o2.tobytes() == out.tobytes())


def test_no_look_up_one_look_up_and_no_plan():
    """P == 0 gives plans and stops only; P == 1; a scalar value goes to every plan; n == 0 is PP_OK"""
    from pathplanning_amd._lib import ptr
    f = fleet()
    s = f.s
    recs, rows = profile(f, which=list(range(6)))
    which = list(range(6))
    none = s.pipe.timetable(s.tickets[which], np.zeros((6, 0)))
    assert none[2].shape == (6, 0) and none[1].shape == (6, 16)
    compare(none, f, which, rows, np.zeros((6, 0)), "length", LIM, 16, "P == 0")
    one = s.pipe.timetable(s.tickets[which], 1.5, by="time")
    assert one[2].shape == (6, 1)
    compare(one, f, which, rows, np.full((6, 1), 1.5), "time", LIM, 16, "P == 1")
    assert one[0].tobytes() == none[0].tobytes() and one[1].tobytes() == none[1].tobytes()
    assert s.pipe.lib.pp_pipeline_timetable(s.pipe.h, 0, None, 0, None, None, None, None, None) == 0
    empty = s.pipe.timetable([], np.zeros((0, 3)))
    assert empty[0].shape == (0,) and empty[2].shape == (0, 3)


def test_beside_queries_in_flight_and_after_a_buffer_grew_the_records_are_the_idle_calls():
    """a call beside eight queries in flight returns the idle call's bytes; so does a call that makes every buffer of the service grow then (more
    plans, more look-ups and more stops than any call before: the outgrown buffers are parked)"""
    f = fleet()
    s = f.s
    lim = V.limits(spacing=0.25, dwell=0.5)
    s.pipe.speed_profile(s.all_tickets, **lim)
    small = np.linspace(0.0, 9.0, 7)
    idle_small = s.pipe.timetable(s.all_tickets[:4], small, by="time", max_stops=2)
    big = np.broadcast_to(np.linspace(-1.0, 45.0, 1531), (N + 2, 1531)).copy()
    flying = s.pipe.submit(s.goals[8:16], s.starts[8:16], np.arange(970, 978, dtype=np.uint64))
    assert len(flying) == 8 and s.pipe.in_flight() == 8
    beside_small = s.pipe.timetable(s.all_tickets[:4], small, by="time", max_stops=2)
    grown = s.pipe.timetable(s.all_tickets, big, by="length", max_stops=333)
    assert s.pipe.in_flight() == 8
    drain(s.pipe, 8)
    s.pipe.release(flying)
    idle = s.pipe.timetable(s.all_tickets, big, by="length", max_stops=333)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(beside_small, idle_small))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(grown, idle))
    assert (grown[0].status[[q for q in range(N) if f.plans[q] is not None]] == 0).all() and grown[2].shape == (N + 2, 1531)
    # two tickets of one query pair under other seeds are plans of their own: each is answered from its own rows
    assert grown[0][N].status == 0 and grown[0][3].status == 0


def test_the_batch_form_equals_the_pipeline_form():
    """HybridAStarBatch.timetable: the same kernel with identity slots on the same queries gives the same bytes; a new batch drops the remembered
    profiles"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError
    f = fleet()
    s = f.s
    n = 16
    batch = pa.HybridAStarBatch(s.val, max_batch=n, max_nodes=32768)
    batch.initialize(s.pipe.nonholo_table())
    res = batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
    assert sum(r.status == 0 for r in res) >= 4
    with pytest.raises(PPError) as e:
        batch.timetable(np.zeros((n, 1)))
    assert e.value.code == PP_ERR_INVALID and "query 0" in str(e.value) and "speed_profile first" in str(e.value)
    lim = V.limits(spacing=0.2, dwell=1.0)
    _, rows = batch.speed_profile(**lim)
    rows = [r if len(r) else None for r in rows]
    s.pipe.speed_profile(s.tickets[:n], **lim)
    for by in ("length", "time"):
        values = mixed(rows, by, 70, lim)
        mine = batch.timetable(values, by=by, max_stops=5)
        theirs = s.pipe.timetable(s.tickets[:n], values, by=by, max_stops=5)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(mine, theirs)), by
        compare(mine, f, range(n), rows, values, by, lim, 5, "batch form by %s" % by)
    some = batch.timetable(values[:5], 5, by="time", max_stops=5)
    assert all(a.tobytes() == b[:5].tobytes() for a, b in zip(some, mine))
    batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
    with pytest.raises(PPError) as e:
        batch.timetable(values, by="time")
    assert "speed_profile first" in str(e.value)
    batch.close()


def test_refusals_launch_nothing_and_leave_the_pipeline_usable():
    """every refusal is PP_ERR_INVALID with the first offending ticket or argument named; after each, the call of before gives the bytes of before"""
    from pathplanning_amd._lib import PPError, TimetableParams, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    pipe.speed_profile(held[:8], samples=False)
    asked = np.linspace(-1.0, 20.0, 9)
    first = pipe.timetable(held[:6], asked, by="time")
    plans, stops, out = np.zeros(128, dtype=TT.PLAN_DTYPE), np.zeros(128 * 16, dtype=TT.STOP_DTYPE), np.zeros(4096, dtype=TT.RESULT_DTYPE)
    good = dict(by=1, max_stops=16, reserved=(0, 0))

    def refused(tickets, *words, n=None, P=2, values=0.5, params=good):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        count = len(t) if n is None else n
        v = None if values is None else np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float64), (len(t), max(P, 0))))
        tp = None
        if params is not None:
            tp = TimetableParams(params["by"], params["max_stops"])
            tp.reserved[0], tp.reserved[1] = params["reserved"]
        rc = lib.pp_pipeline_timetable(pipe.h, count, ptr(t), P, ptr(v), C.byref(tp) if tp is not None else None, ptr(plans), ptr(stops), ptr(out))
        msg = lib.pp_last_error().decode()
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)
        now = pipe.timetable(held[:6], asked, by="time")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(now, first)), msg

    refused((held + held)[:CAPACITY + 1], "capacity")
    refused(held[:1], "capacity", n=-1)
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused([held[0], held[9]], "ticket %d" % held[9], "speed_profile first")  # held, but not in the last speed-profile call
    refused(held[:2], "params", params=None)
    refused(held[:2], "values_host", values=None)
    for bad in (2, -1):
        refused(held[:2], "by", params=dict(good, by=bad))
    for bad in (-1, (1 << 16) + 1):
        refused(held[:2], "max_stops", params=dict(good, max_stops=bad))
    for bad in ((1, 0), (0, -7)):
        refused(held[:2], "reserved", params=dict(good, reserved=bad))
    refused(held[:2], "n_points", P=-1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(held[:3], "ticket %d" % held[1], "not finite", P=3, values=[[0.0, 1.0, 2.0], [0.0, 1.0, bad], [bad, 0.0, 0.0]])
    # n * P > 2^26: refused on the count alone, before a value is read (a buffer of the stated size is still passed)
    t2 = np.ascontiguousarray(held[:2], dtype=np.uint64)
    huge = np.zeros((2, (1 << 25) + 1))
    tp = TimetableParams(1, 16)
    assert lib.pp_pipeline_timetable(pipe.h, 2, ptr(t2), (1 << 25) + 1, ptr(huge), C.byref(tp), None, None, None) == PP_ERR_INVALID
    assert "n_points" in lib.pp_last_error().decode()
    del huge
    # the batch entry on the pipeline's buffer set
    rc = lib.pp_planner_timetable(pipe.planner_h, 1, 1, ptr(np.zeros(1)), C.byref(tp), ptr(plans), ptr(stops), ptr(out))
    assert rc == PP_ERR_INVALID and "pp_pipeline_timetable" in lib.pp_last_error().decode()
    # a query in flight: its ticket is refused; released since the profile: refused too
    flying = pipe.submit(s.goals[8:9], s.starts[8:9], np.array([954], dtype=np.uint64))
    assert len(flying) == 1 and pipe.in_flight() == 1
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "in flight")
    drain(pipe, 1)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "speed_profile first")  # held now, never profiled
    pipe.release(flying)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "released")
    with pytest.raises(PPError) as e:
        pipe.timetable(held[:2], [0.0, np.nan], by="time")
    assert e.value.code == PP_ERR_INVALID
    with pytest.raises(ValueError):
        pipe.timetable(held[:3], np.zeros((2, 4)))
    with pytest.raises(ValueError):
        pipe.timetable(held[:3], 0.0, by="row")
    again = pipe.timetable(held[:6], asked, by="time")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, first))


def test_the_cpp_mirror_equals_a_plain_sequential_loop_over_the_downloaded_rows():
    """tests/cpp/test_pipeline_timetable.cpp: Timetable(tickets, values) of Planner::HybridAStarPipeline against a loop over the rows SpeedProfile returns"""
    import os
    import subprocess
    from pathplanning_amd import build
    exe = build.build_pipeline_timetable_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"Timetable(tickets, values) == the sequential loop over the downloaded rows" in r.stdout
