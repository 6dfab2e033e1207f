"""-m gpu: start delays that clear conflicts between held plans, by priority and ticket (pp_pipeline_deconflict, pp_planner_deconflict; k_delay_level in
pathplanning_amd/csrc/pp_deconflict.hpp; the definition is in include/pp_hip.h).

The comparator is tests/delay_restatement.py, a restatement in numpy that shares nothing with the kernel, fed with the (s, v, t) rows that
speed_profile(samples=True) returned; the plans' edges are rebuilt from get_path_of as tests/test_gpu_pipeline_locate.py rebuilds them.  On a DECIDED
vehicle (no separation of a candidate it tried, nor of a vehicle above it that it can be reached from, lies within 1e-9 of the margin) status,
delay_steps, n_tried and blocker are EQUAL, t_start and t_block are equal bit for bit and s_block agrees within 1e-9.  At most 2 % of a case's
vehicles may be undecided (tests/test_delay_restatement_host.py checks on the CPU that the restatement alone leaves none undecided on the oracle's
plans, over the same margins, starts and pair lists).  In the bit-exact mode the restatement is fed the device's own poses -- conflicts(poses=True)
over the horizon that begins max_delay_steps steps earlier -- and the point disc is the footprint: a delay is an index shift, so EVERY field of
EVERY vehicle is equal.  Independent of any restatement: a conflict call with the returned starts finds every pair of scheduled vehicles clear, and
every vehicle that waited in conflict with its blocker one step earlier.

Scene: the one of tests/test_gpu_pipeline_stamp.py (48 plans held in a capacity-64 pipeline, shared with the other files of that scene).  Every test
leaves the pipeline without a footprint and with nothing in flight."""
import ctypes as C

import numpy as np
import pytest

import conflict_restatement as CR
import delay_restatement as DR
import oracle_lib as O
import speed_restatement as V
from test_conflict_restatement_host import LIM
from test_delay_restatement_host import DS, HOLDS, TS, cases
from test_gpu_pipeline_conflicts import bits, fleet
from test_gpu_pipeline_locate import restated
from test_gpu_pipeline_stamp import CAPACITY, N, Plans, drain

pytestmark = pytest.mark.gpu

PP_ERR_INVALID = -1
TOL = 1e-9
MAX_UNDECIDED = 0.02
NAMES = ["T=%d" % T for T in TS] + ["D=%d" % D for D in DS] + ["chain", "star", "all-12"] + ["nearest, " + h for h in HOLDS] + ["CAR3"]


def compare(got, want, what, exact=False):
    """the device's records (a numpy record array) against the restatement's; returns how many vehicles were undecided"""
    assert len(got) == len(want) and got.dtype.itemsize == 48, what
    undecided = 0
    for i, (a, b) in enumerate(zip(got, want)):
        here = (what, "vehicle", i, a, "want", {k: b[k] for k in ("status", "delay_steps", "n_tried", "blocker", "t_start", "t_block", "s_block", "undecided")})
        if b["undecided"] and not exact:
            undecided += 1
            continue
        assert (a.status, a.delay_steps, a.n_tried, a.blocker) == (b["status"], b["delay_steps"], b["n_tried"], b["blocker"]), here
        assert bits(a.t_start) == bits(b["t_start"]) and bits(a.t_block) == bits(b["t_block"]), here
        if exact:
            assert tuple(a.s_block) == b["s_block"], here
        else:
            assert np.abs(np.asarray(a.s_block) - np.asarray(b["s_block"])).max() <= TOL, here
    print("%s: %d vehicles, %d waited, %d blocked, %d without a plan, %d undecided" % (what, len(got), int((got.delay_steps > 0).sum()), int((got.status == 1).sum()),
                                                                                      int((got.status == -1).sum()), undecided))
    assert undecided <= MAX_UNDECIDED * len(got), what
    return undecided


def call_of(f, name):
    """a case of tests/test_delay_restatement_host.py on the scene's pipeline: its tickets, the device's rows and the call's arguments"""
    which, pairs, t_start, discs, kw = cases(f.s.starts)[name]
    tickets = f.s.tickets[which]
    recs, rows = f.s.pipe.speed_profile(tickets, **LIM)
    return which, pairs, t_start, discs, kw, tickets, recs, rows


def restate(f, which, rows, t_start, pairs, discs, poses=None, **kw):
    return DR.deconflict([f.plans[q] for q in which], [r if len(r) else None for r in rows], t_start, pairs, discs, LIM["a_acc"], LIM["a_dec"], poses=poses, **kw)


def extended_poses(pipe, tickets, t_start, kw):
    """the device's own extended trajectory: the poses of a conflict call whose horizon begins max_delay_steps lattice steps (and half a step) earlier"""
    k0, T = CR.lattice(kw["t_from"], kw["t_to"], kw["dt"])
    D = kw["max_delay_steps"]
    wider = {k: v for k, v in kw.items() if k != "max_delay_steps"}
    wider["t_from"] = (k0 - D - 0.5) * kw["dt"]
    assert CR.lattice(wider["t_from"], wider["t_to"], wider["dt"]) == (k0 - D, T + D)
    return pipe.conflicts(tickets, t_start, poses=True, **wider)[2]


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    """every case of tests/test_delay_restatement_host.py: lattices of 1, 63, 64, 65 and 130 times, largest delays of 0, 1, 63, 64 and 65 steps, a chain
    (as many levels as vehicles), a star, every pair of 12, the 32-nearest list over all 48 plans (a failed query among them) under the four
    combinations of the hold flags, and a three-disc footprint"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows = call_of(f, name)
    car = pa.Footprint(s.ms, discs) if name == "CAR3" else None
    try:
        if car is not None:
            s.pipe.set_footprint(car)
        got = s.pipe.deconflict(tickets, t_start, pairs=pairs, **kw)
    finally:
        if car is not None:
            s.pipe.set_footprint(None)
            car.close()
    _, _, want = restate(f, which, rows, t_start, pairs, discs, **kw)
    compare(got, want, name)
    levels = pa.planner.delay_levels(len(which), pairs)
    assert list(levels) == DR.levels(len(which), pairs)
    if name == "chain":
        assert list(levels) == list(range(16))
    if name == "star":
        assert list(levels) == [0] + [1] * 15 and (got.blocker[got.blocker >= 0] == 0).all()
    if name == "D=0":
        assert set(got.delay_steps) <= {0, -1} and (got.n_tried == 1).all() and (got.status == 1).any()
    if name.startswith("nearest"):
        failed = [q for q in range(N) if recs[q].status != 0]
        assert failed and all(got[q].tobytes() == bytes(C.c_int32(-1)) * 2 + bytes(4) + bytes(C.c_int32(-1)) + bytes(32) for q in failed)
        assert not np.isin(got.blocker, failed).any()  # (ignored by those below)
        assert (got.delay_steps > 0).sum() >= 3 and (got.status == 1).sum() >= 3
    if name == "all-12":
        # pairs == NULL lists every pair; the explicit list, and the same list shuffled and with its pairs turned round, give the same bytes
        every = np.array(CR.all_pairs(12), dtype=np.int32)
        assert s.pipe.deconflict(tickets, t_start, pairs=every, **kw).tobytes() == got.tobytes()
        rng = np.random.default_rng(5)
        shuffled = every[rng.permutation(len(every))]
        shuffled[::2] = shuffled[::2, ::-1].copy()
        assert s.pipe.deconflict(tickets, t_start, pairs=shuffled, **kw).tobytes() == got.tobytes()
        assert s.pipe.deconflict(tickets, t_start, pairs=np.concatenate([shuffled, every[:7]]), **kw).tobytes() == got.tobytes()  # (pairs given twice)
        assert (got.delay_steps > 0).sum() >= 2


@pytest.mark.parametrize("name", ["T=1", "T=65", "D=1", "D=64", "chain", "all-12", "nearest, absent", "nearest, hold-both"])
def test_bit_exact_on_the_devices_own_poses(name):
    """the point disc as the footprint and the restatement fed the device's own extended trajectory: every field of every vehicle is EQUAL, nothing is
    excluded -- and the records are the bytes of the call without a footprint"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows = call_of(f, name)
    plain = s.pipe.deconflict(tickets, t_start, pairs=pairs, **kw)
    point = pa.Footprint(s.ms, s.point)
    try:
        s.pipe.set_footprint(point)
        got = s.pipe.deconflict(tickets, t_start, pairs=pairs, **kw)
        poses = extended_poses(s.pipe, tickets, t_start, kw)
    finally:
        s.pipe.set_footprint(None)
        point.close()
    assert got.tobytes() == plain.tobytes()
    _, _, want = restate(f, which, rows, t_start, pairs, s.point, poses=poses, **kw)
    assert compare(got, want, "bit-exact, " + name, exact=True) == 0


@pytest.mark.parametrize("name", ["D=65", "chain", "nearest, absent", "nearest, hold-after", "CAR3"])
def test_the_returned_starts_are_clear_and_one_step_less_is_not(name):
    """independent of any restatement: a conflict call with the returned starts finds every pair of scheduled vehicles at min_separation >= margin - 1e-9,
    and for every vehicle that waited the same call with one step less finds it closer than margin + 1e-9 to its blocker"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows = call_of(f, name)
    look = {k: v for k, v in kw.items() if k != "max_delay_steps"}
    car = pa.Footprint(s.ms, discs) if name == "CAR3" else None
    try:
        if car is not None:
            s.pipe.set_footprint(car)
        got = s.pipe.deconflict(tickets, t_start, pairs=pairs, **kw)
        ok = np.flatnonzero(got.status == 0)
        index = {int(i): k for k, i in enumerate(ok)}
        listed = CR.all_pairs(len(which)) if pairs is None else pairs
        among = [(index[a], index[b]) for a, b in listed if a in index and b in index]
        assert len(among) >= 5
        found = s.pipe.conflicts(tickets[ok], got.t_start[ok], pairs=among, **look)[1]
        assert all(r.status in (0, 2) and r.min_separation >= kw["margin"] - TOL for r in found), min(r.min_separation for r in found)
        waited = [int(i) for i in ok if got.delay_steps[i] > 0]
        assert len(waited) >= 2
        for i in waited:
            j = int(got.blocker[i])
            assert 0 <= j < i and got.status[j] == 0
            earlier = float(t_start[i]) + float(got.delay_steps[i] - 1) * kw["dt"]
            rec = s.pipe.conflicts(tickets[[j, i]], [got.t_start[j], earlier], **look)[1][0]
            assert rec.n_times > 0 and rec.min_separation < kw["margin"] + TOL, (i, j, rec.min_separation)
    finally:
        if car is not None:
            s.pipe.set_footprint(None)
            car.close()


def test_two_tickets_of_one_query_the_second_waits_or_is_blocked_for_ever():
    """tickets 3 and N are one query (the same start, the same goal): from one start time the second waits d > 0 steps; with hold_after the first
    stands at the goal for ever, and the second finds no clear delay for any D tried"""
    f = fleet()
    s = f.s
    which = [3, N]
    tickets = s.all_tickets[which]
    recs, rows = s.pipe.speed_profile(tickets, **LIM)
    assert recs[0].status == 0 and recs[1].status == 0
    duration = max(float(r.duration) for r in recs)
    for D in (int(duration / 0.1) + 5, int(duration / 0.1) + 40):
        kw = dict(t_from=0.0, t_to=2.0 * duration + 0.1 * D + 5.0, dt=0.1, margin=0.0, max_delay_steps=D)
        got = s.pipe.deconflict(tickets, [1.0, 1.0], **kw)
        _, _, want = restate(f, which, rows, [1.0, 1.0], None, s.point, **kw)
        compare(got, want, "one query twice, D = %d" % D)
        assert (got.status[0], got.delay_steps[0], got.n_tried[0], got.blocker[0], got.t_start[0]) == (0, 0, 1, -1, 1.0)
        d = int(got.delay_steps[1])
        assert got.status[1] == 0 and d > 0 and got.n_tried[1] == d + 1 and got.blocker[1] == 0 and bits(got.t_start[1]) == bits(np.float64(1.0) + np.float64(d) * np.float64(0.1))
        look = {k: v for k, v in kw.items() if k != "max_delay_steps"}
        assert s.pipe.conflicts(tickets, got.t_start, **look)[1][0].status in (0, 2)
        assert s.pipe.conflicts(tickets, [1.0, 1.0 + (d - 1) * 0.1], **look)[1][0].min_separation < TOL
        held = s.pipe.deconflict(tickets, [1.0, 1.0], hold_after=True, **kw)
        compare(held, restate(f, which, rows, [1.0, 1.0], None, s.point, hold_after=True, **kw)[2], "one query twice, held, D = %d" % D)
        assert (held.status[1], held.delay_steps[1], held.n_tried[1], held.blocker[1], held.t_start[1]) == (1, -1, D + 1, 0, 1.0) and held.status[0] == 0
    # starts further apart than the durations: nobody waits
    apart = s.pipe.deconflict(tickets, [1.0, 1.0 + duration + 0.35], **kw)
    assert (apart.status == 0).all() and (apart.delay_steps == 0).all() and (apart.n_tried == 1).all() and (apart.blocker == -1).all()
    assert apart[0].tobytes()[24:] == bytes(24)


def test_a_one_pose_plan_and_a_failed_query():
    """on an open 16 m box with a closed room (tests/test_gpu_pipeline_locate.py's): a goal inside the room (no plan: status -1, ignored by those below),
    start == goal (one pose: present at the one instant u == 0, or standing for ever) and a plan of a few edges beside them in one call"""
    import pathplanning_amd as pa
    w = O.World(lower=(-8.0, -8.0, -np.pi), upper=(8.0, 8.0, np.pi), resolution=0.1)
    for dx, dy, pose in ((4.3, 0.3, (4.0, 2.0, 0.0)), (4.3, 0.3, (4.0, 6.0, 0.0)), (0.3, 4.3, (2.0, 4.0, 0.0)), (0.3, 4.3, (6.0, 4.0, 0.0))):
        w.add_rectangle(dx, dy, pose)
    w.update()
    ctx = pa.Context(0)
    ms = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, 0.1)
    ms.upload_dist2(w.d2())
    ms.upload_occupancy(w.occ())
    ms.upload_path_cost(w.pathcost())
    val = pa.StateValidatorOccupancyMap(ms)
    # the third plan drives through the second one's only pose
    starts = np.array([(-5.0, -5.0, 0.0), (-3.03, 0.04, 0.0), (-5.03, 0.04, 0.0)])
    goals = np.array([(4.0, 4.0, 0.0), (-3.03, 0.04, 0.0), (-1.03, 0.04, 0.0)])
    pipe = pa.HybridAStarPipeline(val, capacity=4, max_nodes=32768, search_rows=4)
    pipe.initialize()
    tickets = pipe.submit(starts, goals, [50, 51, 52])
    res = drain(pipe, 3)
    assert [res[int(t)].status for t in tickets] == [-1, 0, 0] and res[int(tickets[1])].n_path == 1
    plans = restated(Plans([None] + [pipe.get_path_of(t) for t in tickets[1:]], goals, ctx))
    lim = V.limits()
    with pytest.raises(pa._lib.PPError) as e:  # no speed_profile yet
        pipe.deconflict(tickets, [0.0, 0.0, 0.0], max_delay_steps=3)
    assert e.value.code == PP_ERR_INVALID and "speed_profile first" in str(e.value) and "ticket %d" % int(tickets[0]) in str(e.value)
    recs, rows = pipe.speed_profile(tickets, **lim)
    assert [r.status for r in recs] == [-1, 0, 0] and recs[1].n_samples == 1
    point = [(0.0, 0.0, float(val.min_safe_radius))]
    for hold in ((False, False), (True, True)):
        for t_start in ([0.0, 1.5, 0.0], [0.0, 1.5, 1.0]):
            kw = dict(t_from=0.0, t_to=8.0, dt=0.5, margin=0.25, hold_before=hold[0], hold_after=hold[1], max_delay_steps=6)
            got = pipe.deconflict(tickets, t_start, **kw)
            _, _, want = DR.deconflict(plans, [None, rows[1], rows[2]], t_start, None, point, lim["a_acc"], lim["a_dec"], **kw)
            compare(got, want, "box, hold %s, starts %s" % (hold, t_start))
            assert got[0].tobytes() == bytes(C.c_int32(-1)) * 2 + bytes(4) + bytes(C.c_int32(-1)) + bytes(32)
            assert (got.status[1], got.delay_steps[1], got.blocker[1]) == (0, 0, -1) and got.blocker[2] in (-1, 1)
            if hold == (True, True):
                assert got.status[2] == 1 and got.n_tried[2] == 7 and got.blocker[2] == 1  # the one-pose plan stands in the way for ever
    pipe.close()


def test_beside_eight_queries_in_flight_the_buffers_grow_and_the_records_are_the_idle_calls():
    """more plans, more columns and more partners than any call before, with eight queries in flight: every buffer of the service grows and the
    outgrown ones are parked; the call reads no map and the records equal the idle call's"""
    f = fleet()
    s = f.s
    s.pipe.speed_profile(s.all_tickets, **LIM)
    t_start = np.concatenate([cases(s.starts)["nearest, absent"][2], [0.0, 2.0]])
    s.pipe.deconflict(s.all_tickets[:2], t_start[:2], t_to=1.0, max_delay_steps=1)
    flying = s.pipe.submit(s.goals[8:16], s.starts[8:16], np.arange(970, 978, dtype=np.uint64))
    assert len(flying) == 8 and s.pipe.in_flight() == 8
    kw = dict(t_from=-5.01, t_to=30.01, dt=0.05, margin=0.5, max_delay_steps=150)
    grown = s.pipe.deconflict(s.all_tickets, t_start, **kw)
    assert s.pipe.in_flight() == 8
    drain(s.pipe, 8)
    s.pipe.release(flying)
    idle = s.pipe.deconflict(s.all_tickets, t_start, **kw)
    assert grown.tobytes() == idle.tobytes() and len(grown) == N + 2 and (grown.delay_steps > 0).sum() >= 3
    # a conflict call afterwards, in the buffers the delay call has grown, is what it is without one
    look = dict(t_from=0.0, t_to=12.95, dt=0.1, margin=0.5)
    a = s.pipe.conflicts(s.tickets, t_start[:N], **look)
    s.pipe.deconflict(s.tickets[:5], t_start[:5], max_delay_steps=2, **look)
    b = s.pipe.conflicts(s.tickets, t_start[:N], **look)
    assert [bytes(r) for r in a[0] + a[1]] == [bytes(r) for r in b[0] + b[1]]


def test_null_outputs_one_plan_and_no_plan():
    """results_host may be NULL; n == 1 has no pair; n == 0 is PP_OK"""
    from pathplanning_amd._lib import ConflictParams, DelayParams, DelayResult, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    pipe.speed_profile(s.tickets[:4], samples=False)
    t = np.ascontiguousarray(s.tickets[:4], dtype=np.uint64)
    ts = np.array([0.0, 0.5, 1.0, 1.5])
    dp = DelayParams(ConflictParams(0.0, 6.35, 0.1, 0.5, 0, 0), 20, 0)
    out = (DelayResult * 4)()
    assert lib.pp_pipeline_deconflict(pipe.h, 4, ptr(t), ptr(ts), 6, None, C.byref(dp), out) == 0
    assert lib.pp_pipeline_deconflict(pipe.h, 4, ptr(t), ptr(ts), 6, None, C.byref(dp), None) == 0
    wrapped = pipe.deconflict(s.tickets[:4], ts, t_to=6.35, margin=0.5, max_delay_steps=20)
    assert bytes(out) == wrapped.tobytes() and [r.status for r in out] == list(wrapped.status)
    one = pipe.deconflict(s.tickets[:1], [0.0], t_to=6.35, max_delay_steps=20)
    assert len(one) == 1 and one.tobytes() == wrapped[:1].tobytes() and (one.status[0], one.delay_steps[0], one.n_tried[0], one.blocker[0]) == (0, 0, 1, -1)
    assert lib.pp_pipeline_deconflict(pipe.h, 1, ptr(t), ptr(ts), 0, None, C.byref(dp), None) == 0
    assert lib.pp_pipeline_deconflict(pipe.h, 0, None, None, 0, None, None, None) == 0
    none = pipe.deconflict([], [])
    assert len(none) == 0 and none.dtype.itemsize == 48
    # an empty pair list: nobody has a partner, nobody waits, one level
    alone = pipe.deconflict(s.tickets[:4], ts, pairs=[], t_to=6.35, margin=0.5, max_delay_steps=20)
    assert (alone.status == 0).all() and (alone.delay_steps == 0).all() and (alone.blocker == -1).all() and np.array_equal(bits(alone.t_start), bits(ts))


def test_refusals_launch_nothing_and_leave_the_pipeline_usable():
    """every refusal of the conflict call and the delay call's own are PP_ERR_INVALID with the first offending ticket or argument named; a valid call
    afterwards gives the records of before; a released ticket is refused afterwards by whichever route it was released"""
    from pathplanning_amd._lib import ConflictParams, DelayParams, DelayResult, PPError, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    pipe.speed_profile(held[:8], samples=False)
    first = pipe.deconflict(held[:6], np.arange(6.0) * 0.1, t_to=10.0, margin=0.5, max_delay_steps=30)
    out = (DelayResult * 128)()
    good = dict(t_from=0.0, t_to=10.0, dt=0.1, margin=0.5, hold_before=0, hold_after=0, max_delay_steps=30, reserved=0)

    def refused(tickets, *words, n=None, ts=0.0, n_pairs=None, pairs=None, params=good):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        count = len(t) if n is None else n
        ts = None if ts is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ts, dtype=np.float64), (len(t),)))
        pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        np_ = (len(t) * (len(t) - 1) // 2 if pr is None else len(pr)) if n_pairs is None else n_pairs
        dp = None
        if params is not None:
            dp = DelayParams(ConflictParams(*[params[k] for k in ("t_from", "t_to", "dt", "margin", "hold_before", "hold_after")]), params["max_delay_steps"], params["reserved"])
        rc = lib.pp_pipeline_deconflict(pipe.h, count, ptr(t), ptr(ts), np_, ptr(pr), C.byref(dp) if dp is not None else None, out)
        msg = lib.pp_last_error().decode()
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    # the delay call's own
    refused(held[:2], "max_delay_steps", ">= 0", params=dict(good, max_delay_steps=-1))
    refused(held[:2], "T + max_delay_steps", "1048577", params=dict(good, max_delay_steps=(1 << 20) - 100))  # T = 101
    refused(held[:2], "T + max_delay_steps", params=dict(good, max_delay_steps=2 ** 31 - 1))
    refused(held[:2], "reserved", params=dict(good, reserved=1))
    # the conflict call's
    refused((held + held)[:CAPACITY + 1], "capacity")
    refused(held[:1], "capacity", n=-1)
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused([held[0], held[9]], "ticket %d" % held[9], "speed_profile first")  # held, but not in the last speed-profile call
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
    refused(held[:2], "lattice times", "more than", params=dict(good, dt=1e-300))
    for flag in ("hold_before", "hold_after"):
        for bad in (2, -1):
            refused(held[:2], "hold_before and hold_after", params=dict(good, **{flag: bad}))
    refused(held[:3], "n_pairs", n_pairs=-1)
    refused(held[:3], "n (n - 1) / 2 = 3", n_pairs=2)
    refused(held[:3], "pair 1", "outside", pairs=[(0, 1), (1, 3)])
    refused(held[:3], "pair 0", "outside", pairs=[(-1, 1)])
    refused(held[:3], "pair 2", "itself", pairs=[(0, 1), (1, 2), (2, 2)])
    # the batch entry on the pipeline's buffer set
    dp = DelayParams(ConflictParams(0.0, 10.0, 0.1, 0.5, 0, 0), 30, 0)
    rc = lib.pp_planner_deconflict(pipe.planner_h, 1, ptr(np.zeros(1)), 0, None, C.byref(dp), out)
    assert rc == PP_ERR_INVALID and "pp_pipeline_deconflict" in lib.pp_last_error().decode()
    # a query in flight: its ticket is refused; held but never profiled: refused; released since the profile, by either route: refused, and the rest answers as before
    flying = [int(t) for t in pipe.submit(s.goals[8:10], s.starts[8:10], np.array([954, 955], dtype=np.uint64))]
    assert len(flying) == 2 and pipe.in_flight() == 2
    refused([held[0], flying[0]], "ticket %d" % flying[0], "in flight")
    res = drain(pipe, 2)
    refused([held[0], flying[0]], "ticket %d" % flying[0], "speed_profile first")
    pipe.speed_profile([held[0], held[1]] + flying, samples=False)
    with_them = pipe.deconflict([held[0], held[1]] + flying, [0.0, 0.1, 0.0, 0.0], t_to=10.0, margin=0.5, max_delay_steps=30)
    assert (with_them.status >= -1).all() and with_them[:2].tobytes() == first[:2].tobytes()
    free = pipe.free_slots()
    pipe.release(flying[:1])
    if res[flying[1]].status == 0:
        pipe.get_paths(flying[1:], max_poses=64, release=True)
    else:
        pipe.release(flying[1:])
    assert pipe.free_slots() == free + 2
    for t in flying:
        assert pipe.lib.pp_pipeline_slot_of(pipe.h, C.c_uint64(t)) == -1
        refused([held[0], t], "ticket %d" % t, "released")
        with pytest.raises(PPError) as e:
            pipe.deconflict([t], [0.0], max_delay_steps=3)
        assert e.value.code == PP_ERR_INVALID and "ticket %d" % t in str(e.value)
    assert pipe.deconflict(held[:2], [0.0, 0.1], t_to=10.0, margin=0.5, max_delay_steps=30).tobytes() == first[:2].tobytes()
    with pytest.raises(PPError) as e:
        pipe.deconflict(held[:2], [0.0, 0.0], max_delay_steps=-1)
    assert e.value.code == PP_ERR_INVALID
    with pytest.raises(ValueError):
        pipe.deconflict(held[:3], [1.0, 2.0])
    # everything is as it was (the profile of the first eight is gone: the last speed-profile call replaced it)
    refused(held[:6], "ticket %d" % held[2], "speed_profile first")
    pipe.speed_profile(held[:8], samples=False)
    assert pipe.deconflict(held[:6], np.arange(6.0) * 0.1, t_to=10.0, margin=0.5, max_delay_steps=30).tobytes() == first.tobytes()


def test_the_batch_form_equals_the_pipeline_form():
    """HybridAStarBatch.deconflict: the same kernels with identity slots on the same queries give the same records, field by field; a new batch drops the
    remembered profiles"""
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
        batch.deconflict(np.zeros(n), max_delay_steps=5)
    assert e.value.code == PP_ERR_INVALID and "query 0" in str(e.value) and "speed_profile first" in str(e.value)
    which, pairs, t_start, discs, kw = cases(s.starts)["chain"]
    _, rows = batch.speed_profile(**LIM)
    s.pipe.speed_profile(s.tickets[:n], **LIM)
    for pr in (pairs, None):
        mine = batch.deconflict(t_start, pairs=pr, **kw)
        theirs = s.pipe.deconflict(s.tickets[:n], t_start, pairs=pr, **kw)
        for name in mine.dtype.names:
            assert np.array_equal(mine[name], theirs[name]), name
        assert mine.tobytes() == theirs.tobytes()
        compare(mine, restate(f, range(n), rows, t_start, pr, s.point, **kw)[2], "batch form")
    some = batch.deconflict(t_start[:5], 5, pairs=[(4, 0), (2, 3)], **kw)
    assert len(some) == 5 and (some.status[[0, 1, 2]] == 0).all() and (some.delay_steps[[0, 1, 2]] == 0).all()
    batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
    with pytest.raises(PPError) as e:
        batch.deconflict(t_start, **kw)
    assert "speed_profile first" in str(e.value)
    batch.close()


def test_the_cpp_mirror_finds_the_delays_of_a_plain_sequential_loop():
    """tests/cpp/test_pipeline_deconflict.cpp: Deconflict(tickets, starts) of Planner::HybridAStarPipeline against a loop over the device's own poses"""
    import os
    import subprocess
    from pathplanning_amd import build
    exe = build.build_pipeline_deconflict_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"Deconflict(tickets, starts) == the sequential loop over the device's poses" in r.stdout
