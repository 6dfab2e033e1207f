"""-m gpu: space-time conflicts between held plans, by ticket (pp_pipeline_conflicts, pp_planner_conflicts; k_trajectory_tickets and k_conflict_pairs in
pathplanning_amd/csrc/pp_conflicts.hpp; the definition is in include/pp_hip.h).

The comparator is tests/conflict_restatement.py, a restatement in numpy that shares nothing with the kernels, fed with the (s, v, t) rows that
speed_profile(samples=True) returned, so that the row search and s(u) are bit-exact; the plans' edges are rebuilt from get_path_of as
tests/test_gpu_pipeline_locate.py rebuilds them.  EQUAL: the plan records (status, n_present, first, last; s_enter and s_leave bit for bit) and every
pair's n_times.  Poses agree within 1e-9 and separations within 1e-9 absolute (the device's sin / cos against numpy's, as everywhere in this suite).
On a pair with no UNDECIDED time (|separation - margin| <= 1e-9, or a pose closer than 1e-9 m to a boundary between two Reeds-Shepp motions) status,
n_conflict, t_first and s_first are EQUAL too; t_min and s_min are EQUAL where the restatement's minimum is more than 1e-9 below every separation that
is not bit-equal to it (separations 1e-12 apart cannot order two times that close), and such a pair counts one undecided time otherwise.  At most
footprint_ref.MAX_LEFT_OUT of the pair-times this file compares may be undecided (tests/test_conflict_restatement_host.py checks on the CPU that the
restatement alone stays within that on the oracle's plans, over the same margins and starts).

Scene: the one of tests/test_gpu_pipeline_stamp.py (48 plans held in a capacity-64 pipeline, shared with that file when both run in one process).
Every test leaves the pipeline without a footprint and with nothing in flight."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import conflict_restatement as CR
import footprint_ref as FR
import locate_restatement as R
import oracle_lib as O
import speed_restatement as V
from test_conflict_restatement_host import MARGINS, starts_of
from test_gpu_pipeline_locate import restated
from test_gpu_pipeline_stamp import CAPACITY, N, Plans, drain, scene
from test_locate_restatement_host import cusp_of

pytestmark = pytest.mark.gpu

PP_ERR_INVALID = -1
TOL = 1e-9
TOTAL = [0, 0]  # pair-times compared by this file so far, and how many of them were undecided


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Fleet:
    def __init__(self):
        self.s = scene()
        self.plans = restated(self.s.P)  # all N + 2


@functools.lru_cache(maxsize=None)
def fleet():
    return Fleet()


def compare(got, tau, traj, want, what):
    """the plan records, pair records and (if there) poses of the device against the restatement's; returns (pair-times, undecided pair-times)"""
    plan_recs, pair_recs = got[0], got[1]
    assert len(plan_recs) == len(traj) and len(pair_recs) == len(want), what
    for i, (a, b) in enumerate(zip(plan_recs, traj)):
        assert (a.status, a.n_present, a.first, a.last) == (b["status"], b["n_present"], b["first"], b["last"]), (what, "plan", i, a.status, a.n_present, a.first, a.last, b["status"])
        assert bits(a.s_enter) == bits(b["s_enter"]) and bits(a.s_leave) == bits(b["s_leave"]), (what, "plan", i, a.s_enter, b["s_enter"])
        if len(got) > 2:
            xyt = got[2][i]
            assert xyt.shape == (len(tau), 3) and np.array_equal(np.isnan(xyt), np.isnan(b["poses"])), (what, "plan", i, "present")
            worst = float(np.nanmax(np.abs(xyt - b["poses"]))) if b["present"].any() else 0.0
            assert worst <= TOL, (what, "plan", i, "poses", worst)
    times = undecided = 0
    for p, (a, b) in enumerate(zip(pair_recs, want)):
        here = (what, "pair", p, a.status, a.n_times, a.n_conflict, a.t_first, a.min_separation, a.t_min, "want", b["status"], b["n_times"], b["n_conflict"], b["t_first"],
                b["min_separation"], b["t_min"])
        assert a.n_times == b["n_times"] and a.reserved == 0 and a.reserved1 == 0.0, here
        if b["status"] in (-1, 2):
            assert a.status == b["status"] and bytes(a)[4:40] == bytes(36) and bytes(a)[48:] == bytes(32), here
            assert a.min_separation == (math.inf if b["status"] == 2 else 0.0), here
            continue
        sep = b["separation"]
        rest = sep[bits(sep) != bits(sep.min())]
        min_decided = not len(rest) or rest.min() > sep.min() + CR.EPS
        left = b["undecided"] + (0 if min_decided else 1)
        times += b["n_times"]
        undecided += left
        assert abs(a.min_separation - b["min_separation"]) <= TOL, here
        if min_decided:
            assert a.t_min == b["t_min"] and tuple(a.s_min) == b["s_min"], here
        if b["undecided"] == 0:
            assert (a.status, a.n_conflict, a.t_first, tuple(a.s_first)) == (b["status"], b["n_conflict"], b["t_first"], b["s_first"]), here
        else:
            assert abs(a.n_conflict - b["n_conflict"]) <= b["undecided"], here
    print("%s: %d plans, %d pairs, %d pair-times, %d undecided" % (what, len(plan_recs), len(pair_recs), times, undecided))
    TOTAL[0] += times
    TOTAL[1] += undecided
    return times, undecided


def restate(f, which, rows, t_start, pairs, lim, discs=None, **kw):
    """conflict_restatement.conflicts on the plans `which` with the device's rows"""
    return CR.conflicts([f.plans[q] for q in which], [r if len(r) else None for r in rows], t_start, pairs, f.s.point if discs is None else discs, lim["a_acc"], lim["a_dec"], **kw)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [(False, False), (True, True), (True, False), (False, True)], ids=["absent", "hold-both", "hold-before", "hold-after"])
def test_every_pair_of_the_fleet_and_the_same_pairs_listed_in_shuffled_order(hold):
    """all 48 plans (a failed query among them: -1 propagates to its 47 pairs; plans with a junction cusp and a dwell; plans whose Reeds-Shepp edge
    reverses inside), starts between -3 s and 9 s, 130 lattice times: pairs == NULL (1128 pairs derived on the device) against the restatement, and
    an explicit list of the same pairs in shuffled order gives the same records"""
    f = fleet()
    s = f.s
    lim = V.limits(spacing=0.25, dwell=0.5)
    recs, rows = s.pipe.speed_profile(s.tickets, **lim)
    t_start = starts_of(N)
    kw = dict(t_from=0.0, t_to=12.95, dt=0.1, margin=MARGINS[0], hold_before=hold[0], hold_after=hold[1])
    got = s.pipe.conflicts(s.tickets, t_start, poses=True, **kw)
    tau, traj, want = restate(f, range(N), rows, t_start, None, lim, **kw)
    assert len(tau) == 130 and len(got[1]) == 1128
    compare(got, tau, traj, want, "all pairs, hold %s" % (hold,))
    failed = [q for q in range(N) if recs[q].status != 0]
    assert failed and all(got[0][q].status == -1 for q in failed)
    assert sum(r.status == -1 for r in got[1]) == sum(N - 1 for _ in failed) - len(failed) * (len(failed) - 1) // 2
    assert sum(r.status == 1 for r in got[1]) >= 3 and sum(r.status == 0 for r in got[1]) >= 100
    if hold == (False, False):
        assert sum(r.status == 2 for r in got[1]) >= 1 and (t_start < 0).any()
    junction = [q for q in range(N) if f.plans[q] is not None and any(isinstance(E, R.ArcEdge) and E.backward for E in f.plans[q].edges) and recs[q].n_cusps >= 1]
    inside = [q for q in range(N) if cusp_of(f.plans[q]) is not None]
    assert junction and inside and all(got[0][q].status == 0 for q in junction + inside)
    order = np.random.default_rng(5).permutation(1128)
    every = np.array(CR.all_pairs(N), dtype=np.int32)
    listed = s.pipe.conflicts(s.tickets, t_start, pairs=every[order], **kw)
    assert [bytes(r) for r in listed[1]] == [bytes(got[1][p]) for p in order] and [bytes(r) for r in listed[0]] == [bytes(r) for r in got[0]]


def test_the_trajectory_stands_for_the_dwell_at_a_junction_cusp():
    """a plan with a reverse primitive, dwell 1.5 s: between the arrival at the cusp stop and the departure the poses are one pose, bit for bit"""
    f = fleet()
    s = f.s
    lim = V.limits(spacing=0.25, dwell=1.5)
    recs, rows = s.pipe.speed_profile(s.tickets, **lim)
    found = 0
    for q in range(N):
        if recs[q].status != 0 or recs[q].n_cusps < 1:
            continue
        r = rows[q]
        k = np.flatnonzero((np.diff(r[:, 0]) == 0.0) & (np.diff(r[:, 2]) >= 1.5))
        if not len(k):
            continue
        found += 1
        t0, t1 = r[k[0], 2], r[k[0] + 1, 2]
        kw = dict(t_from=0.0, t_to=float(recs[q].duration), dt=0.05)
        plans, _, xyt = s.pipe.conflicts(s.tickets[q:q + 1], [0.0], poses=True, **kw)
        tau = CR.times(*CR.lattice(kw["t_from"], kw["t_to"], kw["dt"]), kw["dt"])
        standing = xyt[0][(tau >= t0) & (tau <= t1)]
        assert len(standing) >= 29 and (bits(standing) == bits(standing[0])).all(), q
        assert plans[0].status == 0 and plans[0].n_present == len(tau)
        compare((plans, [], xyt), tau, restate(f, [q], [r], [0.0], [], lim, **kw)[1], [], "dwell, plan %d" % q)
        if found == 3:
            break
    assert found >= 1


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_lattices_that_end_in_fill_and_pass_a_block_of_64(T):
    """T lattice times from a lattice point that is not 0 (k0 = 7): one partial block, one full block, a block of one time behind a full one, two full
    blocks and two times"""
    f = fleet()
    s = f.s
    lim = V.limits(spacing=0.5)
    which = list(range(12))
    _, rows = s.pipe.speed_profile(s.tickets[which], **lim)
    t_start = starts_of(12) * 0.25
    kw = dict(t_from=0.7 - 1e-9, t_to=0.1 * (7 + T - 1) + 0.05, dt=0.1, margin=MARGINS[1], hold_before=True)
    assert CR.lattice(kw["t_from"], kw["t_to"], kw["dt"]) == (7, T)
    got = s.pipe.conflicts(s.tickets[which], t_start, poses=True, **kw)
    tau, traj, want = restate(f, which, rows, t_start, None, lim, **kw)
    compare(got, tau, traj, want, "T = %d" % T)
    assert len(got[2][0]) == T and len(got[1]) == 66


def test_profiles_of_1_64_and_65_rows_and_windowed_profiles():
    """N == 1 (the window [0, 0]: the vehicle is present at one instant, or for ever under the hold flags), N == 64 and N == 65 (the row search over a
    full block and one more), each by a spacing found for some plan; and profiles of a window 3 m .. 9 m: s_enter is the window's first sample"""
    f = fleet()
    s = f.s
    for what, wanted in (("N == 64", lambda n: n == 64), ("N == 65", lambda n: n == 65)):
        q, spacing, n = V.find_spacing(f.plans[:N], wanted)
        other = (q + 1) % N if f.plans[(q + 1) % N] is not None else (q + 2) % N
        lim = V.limits(spacing=spacing)
        recs, rows = s.pipe.speed_profile(s.tickets[[q, other]], **lim)
        assert recs[0].n_samples == n
        kw = dict(t_from=-2.0, t_to=40.0, dt=0.25, margin=MARGINS[2])
        got = s.pipe.conflicts(s.tickets[[q, other]], [0.0, 1.0], poses=True, **kw)
        compare(got, *restate(f, [q, other], rows, [0.0, 1.0], None, lim, **kw), "%s: plan %d at spacing %g" % (what, q, spacing))
    which = [q for q in range(N) if f.plans[q] is not None and f.plans[q].edges][:6]
    lim = V.limits(spacing=0.3)
    recs, rows = s.pipe.speed_profile(s.tickets[which], to_length=0.0, **lim)
    assert any(r.n_samples == 1 for r in recs)
    for hold in ((False, False), (True, True)):
        kw = dict(t_from=-1.0, t_to=1.0, dt=0.5, margin=0.0, hold_before=hold[0], hold_after=hold[1])
        starts = [0.0, 0.5, 0.25, 0.0, -0.5, 1.0]
        got = s.pipe.conflicts(s.tickets[which], starts, poses=True, **kw)
        compare(got, *restate(f, which, rows, starts, None, lim, **kw), "N == 1, hold %s" % (hold,))
        one = next(i for i, r in enumerate(recs) if r.n_samples == 1)
        assert got[0][one].n_present == (5 if hold[0] else 1) or starts[one] == 0.25
    recs, rows = s.pipe.speed_profile(s.tickets[which], from_length=3.0, to_length=9.0, v_start=2.0, v_end=1.0, **lim)
    kw = dict(t_from=0.0, t_to=8.0, dt=0.125, margin=MARGINS[0])
    got = s.pipe.conflicts(s.tickets[which], np.zeros(6), poses=True, **kw)
    compare(got, *restate(f, which, rows, np.zeros(6), None, lim, **kw), "windowed profiles")
    assert all(a.s_enter == r.s_first and a.first == 0 for a, r in zip(got[0], recs) if r.status == 0)


def test_a_one_pose_plan_and_a_failed_query():
    """on an open 16 m box with a closed room (tests/test_gpu_pipeline_locate.py's): a goal inside the room (no plan: -1 propagates to its pairs), start
    == goal (one pose: present at the one instant u == 0, or standing for ever) and a plan of a few edges beside them in one call"""
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
    starts = np.array([(-5.0, -5.0, 0.0), (-5.03, 3.04, 0.4), (-5.03, 0.04, 0.0)])
    goals = np.array([(4.0, 4.0, 0.0), (-5.03, 3.04, 0.4), (-2.53, 0.04, 0.0)])
    pipe = pa.HybridAStarPipeline(val, capacity=4, max_nodes=32768, search_rows=4)
    pipe.initialize()
    tickets = pipe.submit(starts, goals, [50, 51, 52])
    res = drain(pipe, 3)
    assert [res[int(t)].status for t in tickets] == [-1, 0, 0] and res[int(tickets[1])].n_path == 1
    plans = restated(Plans([None] + [pipe.get_path_of(t) for t in tickets[1:]], goals, ctx))
    lim = V.limits()
    with pytest.raises(pa._lib.PPError) as e:  # no speed_profile yet
        pipe.conflicts(tickets, [0.0, 0.0, 0.0])
    assert e.value.code == PP_ERR_INVALID and "speed_profile first" in str(e.value) and "ticket %d" % int(tickets[0]) in str(e.value)
    recs, rows = pipe.speed_profile(tickets, **lim)
    assert [r.status for r in recs] == [-1, 0, 0] and recs[1].n_samples == 1
    point = [(0.0, 0.0, float(val.min_safe_radius))]
    for hold in ((False, False), (True, True)):
        kw = dict(t_from=0.0, t_to=6.0, dt=0.5, margin=0.25, hold_before=hold[0], hold_after=hold[1])
        t_start = [0.0, 1.5, 0.0]
        got = pipe.conflicts(tickets, t_start, poses=True, **kw)
        tau, traj, want = CR.conflicts(plans, [None, rows[1], rows[2]], t_start, None, point, lim["a_acc"], lim["a_dec"], **kw)
        compare(got, tau, traj, want, "box, hold %s" % (hold,))
        assert [r.status for r in got[1]] == [-1, -1, want[2]["status"]] and bytes(got[1][0]) == bytes(C.c_int32(-1)) + bytes(76)
        assert bytes(got[0][0]) == bytes(C.c_int32(-1)) + bytes(4) + 2 * bytes(C.c_int32(-1)) + bytes(16) and np.isnan(got[2][0]).all()
        assert got[0][1].n_present == (13 if hold[0] else 1) and got[0][1].s_enter == 0.0
    pipe.close()


def test_the_point_disc_as_a_footprint_and_a_three_disc_footprint():
    """no footprint (the map's min_safe_radius as a disc) and the same disc given as a footprint give the same bytes; the three-disc CAR3 against the
    restatement (the centres need the heading's sin and cos, which the trajectory carries)"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    lim = V.limits(spacing=0.25)
    which = list(range(24))
    _, rows = s.pipe.speed_profile(s.tickets[which], **lim)
    t_start = starts_of(24) * 0.5
    kw = dict(t_from=0.0, t_to=9.9, dt=0.15, margin=MARGINS[1], hold_after=True)
    none = s.pipe.conflicts(s.tickets[which], t_start, poses=True, **kw)
    point, car = pa.Footprint(s.ms, s.point), pa.Footprint(s.ms, FR.CAR3)
    try:
        s.pipe.set_footprint(point)
        as_disc = s.pipe.conflicts(s.tickets[which], t_start, poses=True, **kw)
        assert [bytes(r) for r in as_disc[0]] == [bytes(r) for r in none[0]] and [bytes(r) for r in as_disc[1]] == [bytes(r) for r in none[1]]
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(as_disc[2], none[2]))
        s.pipe.set_footprint(car)
        got = s.pipe.conflicts(s.tickets[which], t_start, poses=True, **kw)
        tau, traj, want = restate(f, which, rows, t_start, None, lim, discs=FR.CAR3, **kw)
        compare(got, tau, traj, want, "CAR3")
        assert any(a.min_separation != b.min_separation for a, b in zip(got[1], none[1]) if a.status >= 0 and a.n_times)
    finally:
        s.pipe.set_footprint(None)
        point.close()
        car.close()
    compare(none, *restate(f, which, rows, t_start, None, lim, **kw), "no footprint")


def test_beside_eight_queries_in_flight_the_buffers_grow_and_the_records_are_the_idle_calls():
    """more plans, more lattice times and more pairs than any call before, with eight queries in flight: every buffer of the service grows and the
    outgrown ones are parked; the call reads no map and the records and poses equal the idle call's"""
    f = fleet()
    s = f.s
    lim = V.limits(spacing=0.25)
    s.pipe.speed_profile(s.all_tickets, **lim)
    t_start = np.concatenate([starts_of(N), [0.0, 2.0]])
    s.pipe.conflicts(s.all_tickets[:2], t_start[:2], t_to=1.0)
    flying = s.pipe.submit(s.goals[8:16], s.starts[8:16], np.arange(960, 968, dtype=np.uint64))
    assert len(flying) == 8 and s.pipe.in_flight() == 8
    kw = dict(t_from=-5.01, t_to=30.01, dt=0.05, margin=MARGINS[0])
    grown = s.pipe.conflicts(s.all_tickets, t_start, poses=True, **kw)
    assert s.pipe.in_flight() == 8
    drain(s.pipe, 8)
    s.pipe.release(flying)
    idle = s.pipe.conflicts(s.all_tickets, t_start, poses=True, **kw)
    assert [bytes(r) for r in grown[0]] == [bytes(r) for r in idle[0]] and [bytes(r) for r in grown[1]] == [bytes(r) for r in idle[1]]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(grown[2], idle[2])) and len(grown[2][0]) == 701
    # two tickets of one query (the same start pose) held before a common start: they stand on each other, 2 R deep, from the first lattice time on
    same = s.pipe.conflicts(s.all_tickets[[3, N]], [1.0, 1.0], hold_before=True, **kw)[1][0]
    assert same.status == 1 and same.n_times >= same.n_conflict >= 120 and same.t_first == same.t_min == -100 * 0.05
    assert same.min_separation == -2.0 * float(np.float32(s.point[0][2])) and tuple(same.s_first) == tuple(same.s_min) == (0.0, 0.0)


def test_null_outputs_one_plan_and_no_plan():
    """each of poses_host, plans_host and results_host may be NULL; n == 1 has no pair; n == 0 is PP_OK"""
    from pathplanning_amd._lib import ConflictParams, ConflictResult, TrajectoryResult, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    pipe.speed_profile(s.tickets[:4], samples=False)
    t = np.ascontiguousarray(s.tickets[:4], dtype=np.uint64)
    ts = np.array([0.0, 0.5, 1.0, 1.5])
    cp = ConflictParams(0.0, 6.35, 0.1, 0.5, 0, 0)
    plans, out, xyt = (TrajectoryResult * 4)(), (ConflictResult * 6)(), np.full((4, 64, 3), -7.0)
    assert lib.pp_pipeline_conflicts(pipe.h, 4, ptr(t), ptr(ts), 6, None, C.byref(cp), ptr(xyt), plans, out) == 0
    full = ([bytes(r) for r in plans], [bytes(r) for r in out], xyt.copy())
    assert (xyt != -7.0).all()
    for mask in range(7):
        plans, out, xyt = (TrajectoryResult * 4)(), (ConflictResult * 6)(), np.full((4, 64, 3), -7.0)
        a, b, c = mask & 1, mask & 2, mask & 4
        assert lib.pp_pipeline_conflicts(pipe.h, 4, ptr(t), ptr(ts), 6, None, C.byref(cp), ptr(xyt) if a else None, plans if b else None, out if c else None) == 0
        assert not a or np.array_equal(bits(xyt), bits(full[2]))
        assert not b or [bytes(r) for r in plans] == full[0]
        assert not c or [bytes(r) for r in out] == full[1]
    got = pipe.conflicts(s.tickets[:1], [0.0], poses=True, t_to=6.35)
    assert len(got[0]) == 1 and got[1] == [] and bytes(got[0][0]) == bytes(pipe.conflicts(s.tickets[:4], [0.0, 0.5, 1.0, 1.5], t_to=6.35)[0][0])
    assert lib.pp_pipeline_conflicts(pipe.h, 1, ptr(t), ptr(ts), 0, None, C.byref(cp), None, None, None) == 0
    assert lib.pp_pipeline_conflicts(pipe.h, 0, None, None, 0, None, None, None, None, None) == 0
    assert pipe.conflicts([], []) == ([], [])
    # a horizon before every start: never both present
    early = pipe.conflicts(s.tickets[:4], [0.0, 0.5, 1.0, 1.5], t_from=-9.0, t_to=-1.0)
    assert all(r.status == 1 and (r.first, r.last) == (-1, -1) for r in early[0]) and all(r.status == 2 and r.min_separation == math.inf for r in early[1])


def test_refusals_launch_nothing_and_leave_the_pipeline_usable():
    """every refusal is PP_ERR_INVALID with the first offending ticket or argument named; a valid call afterwards gives the records of before"""
    from pathplanning_amd._lib import ConflictParams, ConflictResult, PPError, TrajectoryResult, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    pipe.speed_profile(held[:8], samples=False)
    first = pipe.conflicts(held[:6], np.arange(6.0))
    plans, out = (TrajectoryResult * 128)(), (ConflictResult * 4096)()
    good = dict(t_from=0.0, t_to=10.0, dt=0.1, margin=0.5, hold_before=0, hold_after=0)

    def refused(tickets, *words, n=None, ts=0.0, n_pairs=None, pairs=None, params=good):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        count = len(t) if n is None else n
        ts = None if ts is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ts, dtype=np.float64), (len(t),)))
        pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        np_ = (len(t) * (len(t) - 1) // 2 if pr is None else len(pr)) if n_pairs is None else n_pairs
        cp = None if params is None else ConflictParams(*[params[k] for k in ("t_from", "t_to", "dt", "margin", "hold_before", "hold_after")])
        rc = lib.pp_pipeline_conflicts(pipe.h, count, ptr(t), ptr(ts), np_, ptr(pr), C.byref(cp) if cp is not None else None, None, plans, out)
        msg = lib.pp_last_error().decode()
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

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
    cp = ConflictParams(0.0, 10.0, 0.1, 0.5, 0, 0)
    rc = lib.pp_planner_conflicts(pipe.planner_h, 1, ptr(np.zeros(1)), 0, None, C.byref(cp), None, plans, out)
    assert rc == PP_ERR_INVALID and "pp_pipeline_conflicts" in lib.pp_last_error().decode()
    # a query in flight: its ticket is refused; released since the profile: refused too
    flying = pipe.submit(s.goals[8:9], s.starts[8:9], np.array([953], dtype=np.uint64))
    assert len(flying) == 1 and pipe.in_flight() == 1
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "in flight")
    drain(pipe, 1)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "speed_profile first")  # held now, never profiled
    pipe.speed_profile([held[0], int(flying[0])], samples=False)
    assert pipe.conflicts([held[0], int(flying[0])], [0.0, 0.0])[1][0].status >= 0
    pipe.release(flying)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "released")
    with pytest.raises(PPError) as e:
        pipe.conflicts(held[:2], [0.0, 0.0], dt=0.0)
    assert e.value.code == PP_ERR_INVALID
    with pytest.raises(ValueError):
        pipe.conflicts(held[:3], [1.0, 2.0])
    # everything is as it was (the profile of the first eight is gone: the last speed-profile call replaced it)
    refused(held[:6], "ticket %d" % held[1], "speed_profile first")
    pipe.speed_profile(held[:8], samples=False)
    again = pipe.conflicts(held[:6], np.arange(6.0))
    assert [bytes(r) for r in again[0]] == [bytes(r) for r in first[0]] and [bytes(r) for r in again[1]] == [bytes(r) for r in first[1]]


def test_a_second_speed_profile_call_with_other_limits_changes_the_answer():
    """the trajectories are the LAST speed-profile call's: with half the speed a vehicle is half as far along after the same time (and the restatement,
    fed the new rows and the new limits, agrees)"""
    f = fleet()
    s = f.s
    which = [q for q in range(N) if f.plans[q] is not None and f.plans[q].length > 20.0][:8]
    kw = dict(t_from=0.0, t_to=6.0, dt=0.5, margin=MARGINS[0])
    out = []
    for lim in (V.limits(spacing=0.25), V.limits(spacing=0.25, v_max_forward=2.5, v_max_reverse=1.0, a_acc=0.5, a_dec=0.9)):
        _, rows = s.pipe.speed_profile(s.tickets[which], **lim)
        got = s.pipe.conflicts(s.tickets[which], np.zeros(8), poses=True, **kw)
        compare(got, *restate(f, which, rows, np.zeros(8), None, lim, **kw), "limits %s" % lim["v_max_forward"])
        out.append(got)
    assert all(b.s_leave < a.s_leave for a, b in zip(out[0][0], out[1][0])) and all(a.n_present == b.n_present == 13 for a, b in zip(out[0][0], out[1][0]))


def test_the_batch_form_equals_the_pipeline_form():
    """HybridAStarBatch.conflicts: the same kernels with identity slots on the same queries give the same records and poses, field by field; a new batch
    drops the remembered profiles"""
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
        batch.conflicts(np.zeros(n))
    assert e.value.code == PP_ERR_INVALID and "query 0" in str(e.value) and "speed_profile first" in str(e.value)
    lim = V.limits(spacing=0.2, dwell=1.0)
    t_start = starts_of(n)
    kw = dict(t_from=-1.0, t_to=14.0, dt=0.2, margin=MARGINS[1], hold_before=True)
    _, rows = batch.speed_profile(**lim)
    mine = batch.conflicts(t_start, poses=True, **kw)
    s.pipe.speed_profile(s.tickets[:n], **lim)
    theirs = s.pipe.conflicts(s.tickets[:n], t_start, poses=True, **kw)
    for a, b in zip(mine[0] + mine[1], theirs[0] + theirs[1]):
        for name, _ in a._fields_:
            x, y = getattr(a, name), getattr(b, name)
            assert (list(x) == list(y)) if hasattr(x, "__len__") else (x == y), name
        assert bytes(a) == bytes(b)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(mine[2], theirs[2]))
    compare(mine, *restate(f, range(n), rows, t_start, None, lim, **kw), "batch form")
    some = batch.conflicts(t_start[:5], 5, pairs=[(4, 0), (2, 3)], **kw)
    every = CR.all_pairs(n)
    assert bytes(some[1][1]) == bytes(mine[1][every.index((2, 3))]) and some[1][0].n_times == mine[1][every.index((0, 4))].n_times
    batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
    with pytest.raises(PPError) as e:
        batch.conflicts(t_start, **kw)
    assert "speed_profile first" in str(e.value)
    batch.close()


def test_the_cpp_mirror_finds_the_conflicts_of_a_plain_sequential_loop():
    """tests/cpp/test_pipeline_conflicts.cpp: Conflicts(tickets, starts) of Planner::HybridAStarPipeline against a loop over the profile's samples"""
    import os
    import subprocess
    from pathplanning_amd import build
    exe = build.build_pipeline_conflicts_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"Conflicts(tickets, starts) == the loop over the profile's samples" in r.stdout


def test_the_share_of_undecided_pair_times_over_all_comparisons():
    """every comparison of this file so far: at most footprint_ref.MAX_LEFT_OUT of the pair-times were undecided"""
    print("%d pair-times compared, %d undecided" % tuple(TOTAL))
    assert TOTAL[0] >= 20000 and TOTAL[1] <= FR.MAX_LEFT_OUT * TOTAL[0]
