"""-m gpu: waits at the start or at a timetable's stops that clear conflicts between held plans, by priority and ticket (pp_pipeline_deconflict_waits,
pp_planner_deconflict_waits; k_wait_places and k_wait_level in pathplanning_amd/csrc/pp_waits.hpp; the definition is in include/pp_hip.h).

The comparator is tests/wait_restatement.py, a restatement in numpy that shares nothing with the kernels and evaluates EVERY candidate (the kernel
takes the header's shortcut), fed with the (s, v, t) rows speed_profile(samples=True) returned.  On a DECIDED vehicle status, place, row, wait_steps,
n_tried and blocker are EQUAL, t_start, t_hold, t_resume and t_block are equal bit for bit and s_wait, s_block agree within 1e-9; at most 2 % of a
case's vehicles may be undecided (tests/test_wait_restatement_host.py checks on the CPU that the restatement alone leaves none undecided on the
oracle's plans over the same cases).  In the bit-exact mode the restatement is fed the device's own extended poses and the returned places, and the
point disc is the footprint: EVERY field of EVERY vehicle is equal.

Scene: the one of tests/test_gpu_pipeline_stamp.py (48 plans held in a capacity-64 pipeline, shared with the other files of that scene).  Every test
leaves the pipeline without a footprint and with nothing in flight."""
import ctypes as C

import numpy as np
import pytest

import conflict_restatement as CR
import wait_restatement as WR
from test_conflict_restatement_host import LIM
from test_gpu_pipeline_conflicts import bits, fleet
from test_gpu_pipeline_deconflict import extended_poses
from test_gpu_pipeline_stamp import CAPACITY, N, drain
from test_wait_restatement_host import wait_cases

pytestmark = pytest.mark.gpu

PP_ERR_INVALID = -1
TOL = 1e-9
MAX_UNDECIDED = 0.02
NAMES = list(wait_cases(np.zeros((N, 3))))
INTS = ("status", "place", "row", "wait_steps", "n_tried", "blocker")
TIMES = ("t_start", "t_hold", "t_resume", "t_block")


def compare(got, want, undecided, what, exact=False):
    """the device's records against the restatement's; returns how many vehicles were undecided"""
    assert len(got) == len(want) and got.dtype.itemsize == 80, what
    left = 0
    for i, (a, b) in enumerate(zip(got, want)):
        here = (what, "vehicle", i, a, "want", b)
        if undecided[i] and not exact:
            left += 1
            continue
        assert all(a[k] == b[k] for k in INTS), here
        assert all(bits(a[k]) == bits(b[k]) for k in TIMES), here
        if exact:
            assert a["s_wait"] == b["s_wait"] and tuple(a["s_block"]) == tuple(b["s_block"]), here
        else:
            assert abs(a["s_wait"] - b["s_wait"]) <= TOL and np.abs(a["s_block"] - b["s_block"]).max() <= TOL, here
    print("%s: %d vehicles, %d wait at the start, %d at a stop, %d blocked, %d without a plan, %d undecided" % (
        what, len(got), int((got.place == -1).sum()), int((got.place >= 0).sum()), int((got.status == 1).sum()), int((got.status == -1).sum()), left))
    assert left <= MAX_UNDECIDED * len(got), what
    return left


def call_of(f, name):
    """a case of tests/test_wait_restatement_host.py on the scene's pipeline: its tickets, the device's rows and the call's arguments"""
    which, pairs, t_start, discs, kw = wait_cases(f.s.starts)[name]
    tickets = f.s.tickets[which]
    recs, rows = f.s.pipe.speed_profile(tickets, **LIM)
    return which, pairs, t_start, discs, kw, tickets, recs, rows


def restate(f, which, rows, t_start, pairs, discs, kw, **more):
    return WR.deconflict_waits([f.plans[q] for q in which], [r if len(r) else None for r in rows], t_start, pairs, discs, LIM["a_acc"], LIM["a_dec"], **dict(kw, **more))


def as_fixed(recs):
    """what pa.planner.wait_fixed makes of a record array, as [n, 2]"""
    bound = np.isin(recs.status, (0, 2))
    return np.stack([np.where(bound, np.where(recs.place >= 0, recs.row, -1), -2), np.where(bound, recs.wait_steps, 0)], axis=1)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    """every case of tests/test_wait_restatement_host.py: lattices of 1, 63, 64, 65 and 130 times, largest waits of 0, 1, 64 and 65 steps, 0, 1 and 4
    places with and without start waits, a chain, a star, every pair of 12, the 32-nearest list over all 48 plans (a failed query among them) under
    the four combinations of the hold flags, and a three-disc footprint; the places are the restatement's too"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows = call_of(f, name)
    car = pa.Footprint(s.ms, discs) if name == "CAR3" else None
    try:
        if car is not None:
            s.pipe.set_footprint(car)
        got, places, counts = s.pipe.deconflict_waits(tickets, t_start, pairs=pairs, places=True, **kw)
        assert s.pipe.deconflict_waits(tickets, t_start, pairs=pairs, **kw).tobytes() == got.tobytes()  # (the same bytes on every run)
    finally:
        if car is not None:
            s.pipe.set_footprint(None)
            car.close()
    _, _, want, undecided, _, spots = restate(f, which, rows, t_start, pairs, discs, kw)
    compare(got, want, undecided, name)
    for i, spot in enumerate(spots):
        if spot is None:
            assert counts[i] == 0
            continue
        mine = places[i][:counts[i]]
        assert counts[i] == len(spot) and np.array_equal(mine.row, spot["row"]) and np.array_equal(mine.column, spot["column"]), (name, i)
        assert np.array_equal(bits(mine.s), bits(spot["s"])) and np.array_equal(bits(mine.t_arrive), bits(spot["t_arrive"])), (name, i)
        if len(spot):
            assert np.abs(mine.pose - spot["pose"]).max() <= TOL and np.abs(mine.sin_theta - spot["sin_theta"]).max() <= TOL and np.abs(mine.cos_theta - spot["cos_theta"]).max() <= TOL
    if "no start" in name:
        assert not (got.place == -1).any() and (got.place >= 0).any()
    if name == "max_places=0":
        plain = s.pipe.deconflict(tickets, t_start, pairs=pairs, **{k: v for k, v in kw.items() if k != "max_places"})
        for mine, theirs in (("status", "status"), ("wait_steps", "delay_steps"), ("n_tried", "n_tried"), ("blocker", "blocker"), ("t_start", "t_start"), ("t_block", "t_block"),
                             ("s_block", "s_block")):
            assert got[mine].tobytes() == plain[theirs].tobytes(), mine
        assert (counts == 0).all() and (got.row == -1).all() and not got.t_hold.any() and not got.t_resume.any() and not got.s_wait.any()
        assert np.array_equal(got.place, np.where(got.wait_steps > 0, -1, -2))


@pytest.mark.parametrize("name", ["T=1", "T=65", "D=1", "D=64", "chain", "all-12, no start", "max_places=1, no start", "max_places=4, no start", "nearest, hold-both"])
def test_bit_exact_on_the_devices_own_poses_and_places(name):
    """the point disc as the footprint, the restatement fed the device's own extended trajectory and places: every field of every vehicle is EQUAL,
    nothing is excluded -- and the records are the bytes of the call without a footprint"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows = call_of(f, name)
    plain = s.pipe.deconflict_waits(tickets, t_start, pairs=pairs, **kw)
    point = pa.Footprint(s.ms, s.point)
    look = {k: v for k, v in kw.items() if k not in ("max_places", "no_start_wait")}
    try:
        s.pipe.set_footprint(point)
        got, places, counts = s.pipe.deconflict_waits(tickets, t_start, pairs=pairs, places=True, **kw)
        poses = extended_poses(s.pipe, tickets, t_start, look)
    finally:
        s.pipe.set_footprint(None)
        point.close()
    assert got.tobytes() == plain.tobytes()
    listed = [places[i][:counts[i]] for i in range(len(which))]
    _, _, want, undecided, _, _ = restate(f, which, rows, t_start, pairs, s.point, kw, poses=poses, listed=listed)
    assert compare(got, want, undecided, "bit-exact, " + name, exact=True) == 0


def test_places_equal_the_trajectory_columns_inside_a_dwell_bit_for_bit():
    """a dwell of 0.37 s on a lattice of 0.1 s: the dwell of every stop that has one holds at least three columns, and at each of them the extended
    trajectory's pose has the bits of the place's standing pose"""
    f = fleet()
    s = f.s
    tickets = s.tickets
    s.pipe.speed_profile(tickets, samples=False, **dict(LIM, dwell=0.37))
    t_start = np.linspace(-2.0, 3.0, N) + 0.0123
    kw = dict(t_from=0.0, t_to=25.0, dt=0.1, max_delay_steps=30)
    got, places, counts = s.pipe.deconflict_waits(tickets, t_start, pairs=[], max_places=8, places=True, **kw)
    poses = extended_poses(s.pipe, tickets, t_start, kw)
    _, stops, _ = s.pipe.timetable(tickets, np.zeros((N, 1)), by="time", max_stops=32)
    k0, T = CR.lattice(kw["t_from"], kw["t_to"], kw["dt"])
    tau = CR.times(k0 - 30, T + 30, kw["dt"])
    checked = 0
    for i in range(N):
        u = tau - np.float64(t_start[i])
        for pl in places[i][:counts[i]]:
            st = stops[i][stops[i].row == pl.row][0]
            assert bits(st.t_arrive) == bits(pl.t_arrive) and bits(st.s) == bits(pl.s)
            assert 30 <= pl.column < T + 30 and u[pl.column] >= pl.t_arrive and not u[pl.column - 1] >= pl.t_arrive
            if not st.t_depart > st.t_arrive:  # (a junction is sampled twice: its second row stands too, arrives when the first departs and does not dwell)
                continue
            inside = np.flatnonzero((u >= st.t_arrive) & (u <= st.t_depart))
            assert len(inside) >= min(3, T + 30 - pl.column) and inside[0] == pl.column
            assert all(poses[i][c].tobytes() == pl.pose.tobytes() for c in inside), (i, pl)
            assert abs(pl.sin_theta - np.sin(pl.pose[2])) < 1e-14 and abs(pl.cos_theta - np.cos(pl.pose[2])) < 1e-14
            checked += 1
    assert checked >= 10 and (got.status[counts > 0] == 0).all()
    s.pipe.speed_profile(tickets, samples=False, **LIM)


def test_a_result_fed_back_as_fixed_is_clear_and_fixed_waits_are_checked_not_decided():
    """the record array of a call as `fixed`: every scheduled vehicle keeps its wait with status 0 and no blocker; a fixed row that is no stop gives -2;
    a fixed wait in conflict gives 2 and the vehicles below still see it; a vehicle already standing at its stop (a < D) is accepted as fixed"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows = call_of(f, "max_places=4, no start")
    first, places, counts = s.pipe.deconflict_waits(tickets, t_start, pairs=pairs, places=True, **kw)
    bound = np.isin(first.status, (0, 2))
    assert (first.place[bound] >= 0).any()
    again = s.pipe.deconflict_waits(tickets, t_start, pairs=pairs, fixed=first, **kw)
    assert np.array_equal(pa.planner.wait_fixed(first, len(first)).view(np.int32).reshape(-1, 2), as_fixed(first))
    assert (again.status[bound] == 0).all() and (again.blocker[bound] == -1).all() and (again.n_tried[bound] == 1).all()
    for name in ("wait_steps", "row", "t_start", "t_hold", "t_resume", "s_wait"):
        assert again[name][bound].tobytes() == first[name][bound].tobytes(), name
    assert np.array_equal(again.place[bound], np.where(first.place[bound] >= 0, 0, first.place[bound]))  # (a fixed vehicle's list is its one row)
    assert again[~bound].tobytes() == first[~bound].tobytes()  # (free again: decided as before)
    # a row that moves: -2, ignored; the restatement agrees on the whole call
    fixed = as_fixed(first)
    waited = int(np.flatnonzero(bound & (first.wait_steps > 0))[0])
    moving = next(q for q in range(waited + 1, len(which)) if bound[q] and rows[q][1, 1] > 0.0)
    fixed[waited] = (-1, 0)
    fixed[moving] = (1, 0)
    other = s.pipe.deconflict_waits(tickets, t_start, pairs=pairs, fixed=fixed, **kw)
    _, _, want, undecided, _, _ = restate(f, which, rows, t_start, pairs, discs, kw, fixed=fixed)
    compare(other, want, undecided, "fixed")
    assert other.status[moving] == -2 and other[moving].tobytes()[4:24] == np.array([-2, -1, -1, 0, -1], dtype=np.int32).tobytes() and other[moving].tobytes()[24:] == bytes(56)
    assert other.status[waited] == 2 and 0 <= other.blocker[waited] < waited and other.wait_steps[waited] == 0 and other.t_block[waited] > 0.0
    # tickets 3, N and N + 1 are one query: the second is bound to the first's start (2) and the third, paired with the second only, still yields to it
    trio = s.all_tickets[[3, N, N + 1]]
    duration = max(float(r.duration) for r in s.pipe.speed_profile(trio, **LIM)[0])
    D = int(duration / 0.1) + 5
    out = s.pipe.deconflict_waits(trio, [1.0, 1.0, 1.0], pairs=[(0, 1), (1, 2)], fixed=[(-1, 0), (-1, 0), (-2, 0)], t_to=2.0 * duration + 0.1 * D + 5.0, max_delay_steps=D)
    assert list(out.status[:2]) == [0, 2] and out.blocker[1] == 0 and out.status[2] == 0 and out.place[2] == -1 and out.wait_steps[2] > 0 and out.blocker[2] == 1
    # already standing: the horizon begins inside the dwell of vehicle q's first inner stop
    s.pipe.speed_profile(tickets, samples=False, **LIM)
    q = int(np.flatnonzero(counts > 0)[0])
    pl = places[q][0]
    standing = dict(t_from=float(t_start[q] + pl.t_arrive + 0.2), t_to=float(t_start[q] + pl.t_arrive + 8.0), dt=0.1, max_delay_steps=6, max_places=4)
    free, free_places, free_counts = s.pipe.deconflict_waits(tickets[[q]], t_start[[q]], places=True, **standing)
    assert pl.row not in free_places[0][:free_counts[0]].row  # (reached before k0: no place of a free vehicle)
    held, held_places, held_counts = s.pipe.deconflict_waits(tickets[[q]], t_start[[q]], fixed=[(pl.row, 3)], places=True, **standing)
    assert held_counts[0] == 1 and held_places[0][0].row == pl.row and held_places[0][0].column < 6
    assert (held.status[0], held.place[0], held.row[0], held.wait_steps[0]) == (0, 0, pl.row, 3) and held.t_hold[0] < standing["t_from"] and held.s_wait[0] == pl.s
    assert bits(held.t_resume[0]) == bits(np.float64(float(CR.lattice(standing["t_from"], standing["t_to"], 0.1)[0] - 6 + int(held_places[0][0].column) + 3)) * np.float64(0.1))


def test_the_batch_form_equals_the_pipeline_form():
    """HybridAStarBatch.deconflict_waits: the same kernels with identity slots on the same queries give the same records and places, field by field"""
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
        batch.deconflict_waits(np.zeros(n), max_delay_steps=5)
    assert e.value.code == PP_ERR_INVALID and "query 0" in str(e.value) and "speed_profile first" in str(e.value)
    which, pairs, t_start, discs, kw = wait_cases(s.starts)["chain"]
    batch.speed_profile(**LIM)
    s.pipe.speed_profile(s.tickets[:n], **LIM)
    for pr, flags in ((pairs, None), (None, np.ones(n, dtype=bool))):
        mine = batch.deconflict_waits(t_start, pairs=pr, no_start_wait=flags, places=True, **kw)
        theirs = s.pipe.deconflict_waits(s.tickets[:n], t_start, pairs=pr, no_start_wait=flags, places=True, **kw)
        for name in mine[0].dtype.names:
            assert np.array_equal(mine[0][name], theirs[0][name]), name
        assert np.array_equal(mine[2], theirs[2])
        for i in range(n):
            assert mine[1][i][:mine[2][i]].tobytes() == theirs[1][i][:theirs[2][i]].tobytes()
    batch.close()


def test_null_outputs_one_plan_and_no_plan():
    """each output may be NULL; n == 1 has no pair; n == 0 is PP_OK"""
    from pathplanning_amd._lib import ConflictParams, DelayParams, WaitParams, WaitPlace, WaitResult, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    pipe.speed_profile(s.tickets[:4], samples=False, **LIM)
    t = np.ascontiguousarray(s.tickets[:4], dtype=np.uint64)
    ts = np.array([0.0, 0.5, 1.0, 1.5])
    wp = WaitParams(DelayParams(ConflictParams(0.0, 6.35, 0.1, 0.5, 0, 0), 20, 0), 2, 0)
    out, spots, counts = (WaitResult * 4)(), (WaitPlace * 8)(), (C.c_int32 * 4)()
    assert lib.pp_pipeline_deconflict_waits(pipe.h, 4, ptr(t), ptr(ts), None, None, 6, None, C.byref(wp), counts, spots, out) == 0
    for outputs in ((None, None, None), (counts, None, None), (None, spots, None), (None, None, out)):
        assert lib.pp_pipeline_deconflict_waits(pipe.h, 4, ptr(t), ptr(ts), None, None, 6, None, C.byref(wp), *outputs) == 0
    wrapped, places, n_places = pipe.deconflict_waits(s.tickets[:4], ts, t_to=6.35, margin=0.5, max_delay_steps=20, max_places=2, places=True)
    assert bytes(out) == wrapped.tobytes() and list(counts) == list(n_places)
    one = pipe.deconflict_waits(s.tickets[:1], [0.0], t_to=6.35, max_delay_steps=20, max_places=2)
    assert len(one) == 1 and one.tobytes() == wrapped[:1].tobytes() and (one.status[0], one.place[0], one.wait_steps[0], one.n_tried[0], one.blocker[0]) == (0, -2, 0, 1, -1)
    assert lib.pp_pipeline_deconflict_waits(pipe.h, 0, None, None, None, None, 0, None, None, None, None, None) == 0
    none = pipe.deconflict_waits([], [])
    assert len(none) == 0 and none.dtype.itemsize == 80
    # rows behind a vehicle's n_places are left as they are
    marked = np.full((4, 2, 64), 7, dtype=np.uint8)
    assert lib.pp_pipeline_deconflict_waits(pipe.h, 4, ptr(t), ptr(ts), None, None, 6, None, C.byref(wp), counts, ptr(marked), None) == 0
    for i in range(4):
        assert (marked[i, counts[i]:] == 7).all() and marked[i, :counts[i]].tobytes() == places[i][:counts[i]].tobytes()


def test_refusals_launch_nothing_and_leave_the_pipeline_usable():
    """every refusal of the delay call and the wait call's own are PP_ERR_INVALID with the first offender named; a valid call afterwards gives the
    records of before"""
    from pathplanning_amd._lib import ConflictParams, DelayParams, PPError, WaitParams, WaitResult, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    pipe.speed_profile(held[:8], samples=False, **LIM)
    first = pipe.deconflict_waits(held[:6], np.arange(6.0) * 0.1, t_to=10.0, margin=0.5, max_delay_steps=30, max_places=4)
    out = (WaitResult * 128)()
    good = dict(t_from=0.0, t_to=10.0, dt=0.1, margin=0.5, hold_before=0, hold_after=0, max_delay_steps=30, reserved=0, max_places=4, reserved2=0)

    def refused(tickets, *words, n=None, ts=0.0, n_pairs=None, pairs=None, params=good, flags=None, fixed=None):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        count = len(t) if n is None else n
        ts = None if ts is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ts, dtype=np.float64), (len(t),)))
        pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        np_ = (len(t) * (len(t) - 1) // 2 if pr is None else len(pr)) if n_pairs is None else n_pairs
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.int32).reshape(-1, 2)
        wp = None
        if params is not None:
            wp = WaitParams(DelayParams(ConflictParams(*[params[k] for k in ("t_from", "t_to", "dt", "margin", "hold_before", "hold_after")]), params["max_delay_steps"],
                                        params["reserved"]), params["max_places"], params["reserved2"])
        rc = lib.pp_pipeline_deconflict_waits(pipe.h, count, ptr(t), ptr(ts), ptr(fl), ptr(fx), np_, ptr(pr), C.byref(wp) if wp is not None else None, None, None, out)
        msg = lib.pp_last_error().decode()
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    # the wait call's own
    refused(held[:2], "max_places", params=dict(good, max_places=-1))
    refused(held[:2], "max_places", "1024", params=dict(good, max_places=1025))
    refused(held[:2], "reserved", params=dict(good, reserved2=1))
    refused(held[:3], "ticket %d" % held[1], "no_start_wait", flags=[0, 2, 1])
    refused(held[:3], "ticket %d" % held[2], "fixed row", fixed=[(-2, 0), (-1, 0), (-3, 0)])
    refused(held[:3], "ticket %d" % held[0], "fixed steps", fixed=[(-1, 31), (-1, 0), (-2, 0)])
    refused(held[:3], "ticket %d" % held[1], "fixed steps", fixed=[(-1, 30), (4, -1), (-2, 0)])
    # the delay call's own
    refused(held[:2], "max_delay_steps", ">= 0", params=dict(good, max_delay_steps=-1))
    refused(held[:2], "T + max_delay_steps", "1048577", params=dict(good, max_delay_steps=(1 << 20) - 100))  # T = 101
    refused(held[:2], "reserved", params=dict(good, reserved=1))
    # the conflict call's
    refused((held + held)[:CAPACITY + 1], "capacity")
    refused(held[:1], "capacity", n=-1)
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused([held[0], held[9]], "ticket %d" % held[9], "speed_profile first")
    refused(held[:2], "t_start", ts=None)
    refused(held[:2], "params", params=None)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(held[:3], "ticket %d" % held[1], "t_start", ts=[0.0, bad, 1.0])
        refused(held[:2], "t_from", params=dict(good, t_from=bad))
        refused(held[:2], "t_to", params=dict(good, t_to=bad))
    refused(held[:2], "t_from <= t_to", params=dict(good, t_from=2.0, t_to=1.0))
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        refused(held[:2], "dt", "> 0", params=dict(good, dt=bad))
    for bad in (-0.01, float("nan"), float("inf")):
        refused(held[:2], "margin", ">= 0", params=dict(good, margin=bad))
    refused(held[:2], "lattice times", "no", params=dict(good, t_from=0.55, t_to=0.55, dt=0.25))
    refused(held[:2], "lattice times", "more than", params=dict(good, t_to=104857.7, dt=0.1))
    for flag in ("hold_before", "hold_after"):
        for bad in (2, -1):
            refused(held[:2], "hold_before and hold_after", params=dict(good, **{flag: bad}))
    refused(held[:3], "n_pairs", n_pairs=-1)
    refused(held[:3], "n (n - 1) / 2 = 3", n_pairs=2)
    refused(held[:3], "pair 1", "outside", pairs=[(0, 1), (1, 3)])
    refused(held[:3], "pair 2", "itself", pairs=[(0, 1), (1, 2), (2, 2)])
    # the batch entry on the pipeline's buffer set
    wp = WaitParams(DelayParams(ConflictParams(0.0, 10.0, 0.1, 0.5, 0, 0), 30, 0), 4, 0)
    rc = lib.pp_planner_deconflict_waits(pipe.planner_h, 1, ptr(np.zeros(1)), None, None, 0, None, C.byref(wp), None, None, out)
    assert rc == PP_ERR_INVALID and "pp_pipeline_deconflict_waits" in lib.pp_last_error().decode()
    # a query in flight: its ticket is refused
    flying = [int(t) for t in pipe.submit(s.goals[8:10], s.starts[8:10], np.array([964, 965], dtype=np.uint64))]
    assert len(flying) == 2 and pipe.in_flight() == 2
    refused([held[0], flying[0]], "ticket %d" % flying[0], "in flight")
    drain(pipe, 2)
    pipe.release(flying)
    refused([held[0], flying[0]], "ticket %d" % flying[0], "released")
    # the wrapper's own checks
    with pytest.raises(PPError) as e:
        pipe.deconflict_waits(held[:2], [0.0, 0.0], max_places=-1)
    assert e.value.code == PP_ERR_INVALID
    with pytest.raises(ValueError):
        pipe.deconflict_waits(held[:3], [1.0, 2.0])
    with pytest.raises(ValueError):
        pipe.deconflict_waits(held[:3], [1.0, 2.0, 3.0], fixed=[(-2, 0)])
    with pytest.raises(ValueError):
        pipe.deconflict_waits(held[:3], [1.0, 2.0, 3.0], no_start_wait=[True])
    # everything is as it was
    assert pipe.deconflict_waits(held[:6], np.arange(6.0) * 0.1, t_to=10.0, margin=0.5, max_delay_steps=30, max_places=4).tobytes() == first.tobytes()


def test_beside_eight_queries_in_flight_the_buffers_grow_and_the_records_are_the_idle_calls():
    """more plans, more columns, more partners and more places than any call before, with eight queries in flight: every buffer of the service grows and
    the outgrown ones are parked; the call reads no map and the records equal the idle call's"""
    f = fleet()
    s = f.s
    s.pipe.speed_profile(s.all_tickets, **LIM)
    t_start = np.concatenate([wait_cases(s.starts)["nearest, absent"][2], [0.0, 2.0]])
    s.pipe.deconflict_waits(s.all_tickets[:2], t_start[:2], t_to=1.0, max_delay_steps=1, max_places=1)
    flying = s.pipe.submit(s.goals[8:16], s.starts[8:16], np.arange(980, 988, dtype=np.uint64))
    assert len(flying) == 8 and s.pipe.in_flight() == 8
    kw = dict(t_from=-5.01, t_to=30.01, dt=0.05, margin=0.5, max_delay_steps=150, max_places=40, places=True, no_start_wait=np.arange(N + 2) % 2 == 1)
    grown = s.pipe.deconflict_waits(s.all_tickets, t_start, **kw)
    assert s.pipe.in_flight() == 8
    drain(s.pipe, 8)
    s.pipe.release(flying)
    idle = s.pipe.deconflict_waits(s.all_tickets, t_start, **kw)
    assert grown[0].tobytes() == idle[0].tobytes() and np.array_equal(grown[2], idle[2]) and len(grown[0]) == N + 2
    assert all(grown[1][i][:grown[2][i]].tobytes() == idle[1][i][:idle[2][i]].tobytes() for i in range(N + 2))
    assert (grown[0].wait_steps > 0).sum() >= 2 and not (grown[0].place[1::2] == -1).any()


@pytest.mark.parametrize("name", ["nearest, absent", "all-12, no start"])
def test_the_broad_phase_at_the_inflated_margin_gives_the_records_of_every_pair(name):
    """a standing pose lies between two trajectory columns, at most one step of v_peak * dt from either: candidate_pairs with its margin increased by
    that step lists every pair that can meet under a wait, and the call over the list gives the records of the call over every pair"""
    f = fleet()
    s = f.s
    which, _, t_start, discs, kw, tickets, recs, rows = call_of(f, name)
    v_peak = max(float(np.asarray(r)[:, 1].max()) for r in rows if len(r))
    look = {k: v for k, v in kw.items() if k in ("t_from", "t_to", "dt", "hold_before", "hold_after")}
    every = s.pipe.deconflict_waits(tickets, t_start, pairs=None, **kw)
    pairs = s.pipe.candidate_pairs(tickets, t_start, times_per_box=16, max_delay_steps=kw["max_delay_steps"], margin=kw["margin"] + v_peak * kw["dt"], **look)[0]
    assert 0 < len(pairs) < len(which) * (len(which) - 1) // 2
    assert s.pipe.deconflict_waits(tickets, t_start, pairs=pairs, **kw).tobytes() == every.tobytes()
    assert (every.wait_steps > 0).any()


def test_the_cpp_mirror_finds_the_waits_of_a_plain_sequential_loop():
    """tests/cpp/test_pipeline_deconflict_waits.cpp: DeconflictWaits(tickets, starts) of Planner::HybridAStarPipeline against a loop over the device's own
    poses and places"""
    import os
    import subprocess
    from pathplanning_amd import build
    exe = build.build_pipeline_deconflict_waits_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"DeconflictWaits(tickets, starts) == the sequential loop over the device's poses and places" in r.stdout
