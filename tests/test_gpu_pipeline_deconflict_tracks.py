"""-m gpu: start delays that clear conflicts and tracked movers (pp_pipeline_deconflict_tracks, pp_planner_deconflict_tracks; k_track_samples,
k_delay_level_tracks and k_track_pairs in pathplanning_amd/csrc/pp_tracks.hpp; the definition is in include/pp_hip.h).

Without tracks the delay records are the BYTES of deconflict().  The comparator is tests/track_restatement.py, a restatement in numpy that shares
nothing with the kernels, fed with the (s, v, t) rows that speed_profile(samples=True) returned and the plans' edges rebuilt from get_path_of; the
tracks of a case are tests/test_track_restatement_host.py's, built from the scene.  On a DECIDED vehicle status, delay_steps, n_tried and blocker are
EQUAL, t_start and t_block are equal bit for bit and s_block agrees within 1e-9; of its track records counts and statuses are equal, t_first and t_min
bit for bit, separations and arc lengths within 1e-9.  At most 2 % of a case's vehicles may be undecided (tests/test_track_restatement_host.py checks on
the CPU that the restatement alone leaves none on the oracle's plans).  In the bit-exact mode the restatement is fed the device's own extended poses and
the point disc is the footprint: EVERY field of both outputs is equal.  Independent of the restatement: a second call with the returned starts, D = 0
and no pairs gives every scheduled, decided vehicle status 0.

Scene: the one of tests/test_gpu_pipeline_stamp.py (48 plans held in a capacity-64 pipeline, shared with the other files of that scene).  Every test
leaves the pipeline without a footprint and with nothing in flight."""
import ctypes as C

import numpy as np
import pytest

import track_restatement as TR
from test_conflict_restatement_host import LIM
from test_delay_restatement_host import cases as delay_cases
from test_gpu_pipeline_conflicts import bits, fleet
from test_gpu_pipeline_deconflict import extended_poses
from test_gpu_pipeline_stamp import CAPACITY, N, drain
from test_track_restatement_host import NAMES, cases, tracks_of

pytestmark = pytest.mark.gpu

PP_ERR_INVALID = -1
TOL = 1e-9
MAX_UNDECIDED = 0.02


def compare(got, got_tracks, want, want_tracks, what, exact=False):
    """the device's delay records and [n, M] track records against the restatement's; returns how many vehicles were undecided"""
    assert len(got) == len(want) and got.dtype.itemsize == 48 and got_tracks.dtype.itemsize == 64, what
    M = len(want_tracks[0]) if want_tracks else 0
    assert got_tracks.shape == (len(want), M), what
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
        for k in range(M):
            t, w = got_tracks[i, k], want_tracks[i][k]
            there = (what, "vehicle", i, "track", k, t, "want", w)
            assert t.reserved == 0 and t.reserved1 == 0.0, there
            if w["undecided"] and not exact:
                continue
            assert (t.status, t.n_times, t.n_conflict) == (w["status"], w["n_times"], w["n_conflict"]), there
            assert bits(t.t_first) == bits(w["t_first"]) and bits(t.t_min) == bits(w["t_min"]), there
            if w["status"] in (-1, 2):
                assert t.tobytes()[4:32] == bytes(28) and t.tobytes()[40:] == bytes(24) and t.min_separation == (np.inf if w["status"] == 2 else 0.0), there
            elif exact:
                assert (t.s_first, t.min_separation, t.s_min) == (w["s_first"], w["min_separation"], w["s_min"]), there
            else:
                assert max(abs(t.s_first - w["s_first"]), abs(t.min_separation - w["min_separation"]), abs(t.s_min - w["s_min"])) <= TOL, there
    n = len(got)
    print("%s: %d vehicles, %d tracks, %d waited, %d blocked, %d without a plan, blocker a track %d, %d undecided" % (
        what, n, M, int((got.delay_steps > 0).sum()), int((got.status == 1).sum()), int((got.status == -1).sum()), int((got.blocker >= n).sum()), undecided))
    assert undecided <= MAX_UNDECIDED * n, what
    return undecided


def call_of(f, name):
    """a case of tests/test_track_restatement_host.py on the scene's pipeline: its tickets, the device's rows, the call's arguments and its tracks"""
    s = f.s
    which, pairs, t_start, discs, kw, M = cases(s.starts)[name]
    tickets = s.tickets[which]
    recs, rows = s.pipe.speed_profile(tickets, **LIM)
    by_plan = {q: (r if len(r) else None) for q, r in zip(which, rows)}
    tracks = tracks_of(f.plans, [by_plan.get(q) for q in range(len(f.plans))], s.starts, s.goals, which, t_start, kw, M)
    return which, pairs, t_start, discs, kw, tickets, recs, rows, tracks


def restate(f, which, rows, t_start, pairs, discs, tracks, poses=None, **kw):
    return TR.deconflict_tracks([f.plans[q] for q in which], [r if len(r) else None for r in rows], t_start, pairs, discs, LIM["a_acc"], LIM["a_dec"], tracks, poses=poses, **kw)


class footprint_of:
    """the pipeline with the footprint `discs` (None: none) for the length of a with block"""

    def __init__(self, s, discs):
        import pathplanning_amd as pa
        self.s, self.fp = s, (pa.Footprint(s.ms, discs) if discs is not None else None)

    def __enter__(self):
        if self.fp is not None:
            self.s.pipe.set_footprint(self.fp)

    def __exit__(self, *exc):
        if self.fp is not None:
            self.s.pipe.set_footprint(None)
            self.fp.close()


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T=1", "T=65", "D=0", "D=64", "chain", "all-12", "nearest, hold-both"])
def test_without_tracks_the_records_are_the_bytes_of_deconflict(name):
    """tracks=None (a NULL track set) and M == 0 (an empty one): k_delay_level_tracks decides what k_delay_level decides, byte for byte"""
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw = delay_cases(s.starts)[name]
    tickets = s.tickets[which]
    s.pipe.speed_profile(tickets, **LIM)
    want = s.pipe.deconflict(tickets, t_start, pairs=pairs, **kw)
    null, recs = s.pipe.deconflict_tracks(tickets, t_start, None, pairs=pairs, **kw)
    empty = s.pipe.deconflict_tracks(tickets, t_start, [], pairs=pairs, details=False, **kw)
    assert null.tobytes() == want.tobytes() and empty.tobytes() == want.tobytes() and recs.shape == (len(which), 0)
    assert (want.status == 0).any() and (name in ("T=1", "D=0") or (want.delay_steps > 0).any())


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    """every case of tests/test_track_restatement_host.py: lattices of 1, 63, 64, 65 and 130 times, largest delays of 0, 1, 64 and 65 steps, 1, 3 and 17
    tracks, no pairs at all, a chain and a star with tracks, the 32-nearest list over all 48 plans (a failed query among them) under the four
    combinations of the hold flags, and a three-disc footprint"""
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows, tracks = call_of(f, name)
    with footprint_of(s, discs if name == "CAR3" else None):
        got, got_tracks = s.pipe.deconflict_tracks(tickets, t_start, tracks, pairs=pairs, **kw)
        only = s.pipe.deconflict_tracks(tickets, t_start, tracks, pairs=pairs, details=False, **kw)
    assert only.tobytes() == got.tobytes()  # (the records do not depend on whether k_track_pairs runs)
    _, _, want, want_tracks = restate(f, which, rows, t_start, pairs, discs, tracks, **kw)
    compare(got, got_tracks, want, want_tracks, name)
    n = len(which)
    track_blocked = got[got.blocker >= n]
    assert (track_blocked.s_block[:, 1] == 0.0).all() and (got.blocker < n + len(tracks)).all()
    if name == "no pairs":
        assert not ((got.blocker >= 0) & (got.blocker < n)).any() and len(track_blocked) >= 1
    if name == "D=0":
        assert set(got.delay_steps) <= {0, -1} and (got.n_tried[got.status >= 0] == 1).all()
    if name.startswith("nearest"):
        failed = [q for q in range(N) if recs[q].status != 0]
        assert failed and all(got[q].tobytes() == bytes(C.c_int32(-1)) * 2 + bytes(4) + bytes(C.c_int32(-1)) + bytes(32) for q in failed)
        assert all(got_tracks[q, k].tobytes() == bytes(C.c_int32(-1)) + bytes(60) for q in failed for k in range(len(tracks)))
    if name in ("chain", "star", "CAR3", "M=17"):
        assert len(track_blocked) >= 1 and ((got.blocker >= 0) & (got.blocker < n)).any()  # a track blocker and a vehicle blocker in one call
    # a scheduled vehicle is clear of every track at its delay; a vehicle blocked by a track for good conflicts with it at the largest delay
    assert np.isin(got_tracks.status[got.status == 0], (0, 2)).all()
    for i in np.flatnonzero((got.status == 1) & (got.blocker >= n)):
        t = got_tracks[i, got.blocker[i] - n]
        assert t.status == 1 and bits(t.t_first) == bits(got.t_block[i]) and t.s_first == got.s_block[i, 0]


@pytest.mark.parametrize("name", ["T=1", "T=65", "D=1", "D=64", "M=17", "chain", "nearest, absent", "nearest, hold-both"])
def test_bit_exact_on_the_devices_own_poses(name):
    """the point disc as the footprint and the restatement fed the device's own extended trajectory: every field of every delay record and of every
    track record is EQUAL, nothing is excluded -- and the records are the bytes of the call without a footprint"""
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows, tracks = call_of(f, name)
    plain, plain_tracks = s.pipe.deconflict_tracks(tickets, t_start, tracks, pairs=pairs, **kw)
    with footprint_of(s, s.point):
        got, got_tracks = s.pipe.deconflict_tracks(tickets, t_start, tracks, pairs=pairs, **kw)
        poses = extended_poses(s.pipe, tickets, t_start, kw)
    assert got.tobytes() == plain.tobytes() and got_tracks.tobytes() == plain_tracks.tobytes()
    _, _, want, want_tracks = restate(f, which, rows, t_start, pairs, s.point, tracks, poses=poses, **kw)
    assert compare(got, got_tracks, want, want_tracks, "bit-exact, " + name, exact=True) == 0


@pytest.mark.parametrize("name", ["D=65", "M=17", "chain", "nearest, hold-after", "CAR3"])
def test_a_plain_check_with_the_returned_starts_finds_every_scheduled_vehicle_clear(name):
    """independent of the restatement: a second call with the returned starts, D = 0 and no pairs gives every scheduled, decided vehicle status 0 (a
    vehicle is decided when no separation of its first call's record lies within 1e-9 of the margin: the second call forms u = tau - t_start' afresh)"""
    f = fleet()
    s = f.s
    which, pairs, t_start, discs, kw, tickets, recs, rows, tracks = call_of(f, name)
    with footprint_of(s, discs if name == "CAR3" else None):
        got, got_tracks = s.pipe.deconflict_tracks(tickets, t_start, tracks, pairs=pairs, **kw)
        again, again_tracks = s.pipe.deconflict_tracks(tickets, got.t_start, tracks, pairs=[], **dict(kw, max_delay_steps=0))
    scheduled = np.flatnonzero(got.status == 0)
    decided = [i for i in scheduled if (np.abs(got_tracks.min_separation[i] - kw["margin"]) > TOL).all()]
    # (tests/test_track_restatement_host.py prints the counts: the case with the fewest scheduled vehicles, M=17, has three, and all three waited)
    assert len(decided) >= 0.98 * len(scheduled) and len(scheduled) >= 3 and (got.delay_steps[scheduled] > 0).any()
    assert (again.status[decided] == 0).all() and (again.delay_steps[decided] == 0).all() and (again.blocker[decided] == -1).all()
    assert np.isin(again_tracks.status[decided], (0, 2)).all()
    assert np.array_equal(again_tracks.n_times[decided], got_tracks.n_times[decided])
    both = again_tracks.n_times[decided] > 0  # (+inf where never both present)
    assert np.abs(again_tracks.min_separation[decided][both] - got_tracks.min_separation[decided][both]).max(initial=0.0) <= TOL


def test_null_outputs_one_plan_and_no_plan():
    """results_host and track_results_host may be NULL, each alone; n == 1 has no pair; n == 0 is PP_OK whatever the tracks"""
    from pathplanning_amd._lib import ConflictParams, DelayParams, DelayResult, TrackResult, TrackSet, ptr
    from pathplanning_amd.planner import track_set
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    pipe.speed_profile(s.tickets[:4], samples=False)
    t = np.ascontiguousarray(s.tickets[:4], dtype=np.uint64)
    ts = np.array([0.0, 0.5, 1.0, 1.5])
    tracks = [(0.3, [(0.0, *s.goals[1][:2]), (7.0, *s.goals[1][:2])]), (1.0, [(2.0, *s.starts[2][:2])])]
    tk, keep = track_set(tracks)
    dp = DelayParams(ConflictParams(0.0, 6.35, 0.1, 0.5, 0, 0), 20, 0)
    out, rec = (DelayResult * 4)(), (TrackResult * 8)()
    assert lib.pp_pipeline_deconflict_tracks(pipe.h, 4, ptr(t), ptr(ts), 6, None, C.byref(dp), C.byref(tk), out, rec) == 0
    wrapped, wrapped_tracks = pipe.deconflict_tracks(s.tickets[:4], ts, tracks, t_to=6.35, margin=0.5, max_delay_steps=20)
    assert bytes(out) == wrapped.tobytes() and bytes(rec) == wrapped_tracks.tobytes() and wrapped_tracks.shape == (4, 2)
    only_tracks = (TrackResult * 8)()
    assert lib.pp_pipeline_deconflict_tracks(pipe.h, 4, ptr(t), ptr(ts), 6, None, C.byref(dp), C.byref(tk), None, only_tracks) == 0
    only_delays = (DelayResult * 4)()
    assert lib.pp_pipeline_deconflict_tracks(pipe.h, 4, ptr(t), ptr(ts), 6, None, C.byref(dp), C.byref(tk), only_delays, None) == 0
    assert lib.pp_pipeline_deconflict_tracks(pipe.h, 4, ptr(t), ptr(ts), 6, None, C.byref(dp), C.byref(tk), None, None) == 0
    assert bytes(only_tracks) == bytes(rec) and bytes(only_delays) == bytes(out)
    assert (wrapped.blocker < 4 + 2).all() and (wrapped.s_block[wrapped.blocker >= 4, 1] == 0.0).all()
    one, one_tracks = pipe.deconflict_tracks(s.tickets[:1], [0.0], tracks, t_to=6.35, margin=0.5, max_delay_steps=20)
    assert len(one) == 1 and one.tobytes() == wrapped[:1].tobytes() and one_tracks.tobytes() == wrapped_tracks[:1].tobytes()
    assert lib.pp_pipeline_deconflict_tracks(pipe.h, 1, ptr(t), ptr(ts), 0, None, C.byref(dp), C.byref(tk), None, None) == 0
    assert lib.pp_pipeline_deconflict_tracks(pipe.h, 0, None, None, 0, None, None, None, None, None) == 0
    broken = TrackSet(3, 1, None, None, None)  # n == 0 is PP_OK whatever the tracks
    assert lib.pp_pipeline_deconflict_tracks(pipe.h, 0, None, None, 0, None, C.byref(dp), C.byref(broken), None, None) == 0
    none, none_tracks = pipe.deconflict_tracks([], [], tracks)
    assert len(none) == 0 and none.dtype.itemsize == 48 and none_tracks.shape == (0, 2) and none_tracks.dtype.itemsize == 64
    del keep


def test_beside_eight_queries_in_flight_the_buffers_grow_and_the_records_are_the_idle_calls():
    """more plans, more columns, more tracks, more waypoints and more records than any call before, with eight queries in flight: every buffer of the
    service grows and the outgrown ones are parked; the call reads no map and the records equal the idle call's"""
    f = fleet()
    s = f.s
    s.pipe.speed_profile(s.all_tickets, **LIM)
    t_start = np.concatenate([delay_cases(s.starts)["nearest, absent"][2], [0.0, 2.0]])
    small = [(0.3, [(0.0, *s.goals[0][:2]), (1.0, *s.goals[0][:2])])]
    s.pipe.deconflict_tracks(s.all_tickets[:2], t_start[:2], small, t_to=1.0, max_delay_steps=1)
    flying = s.pipe.submit(s.goals[8:16], s.starts[8:16], np.arange(980, 988, dtype=np.uint64))
    assert len(flying) == 8 and s.pipe.in_flight() == 8
    kw = dict(t_from=-5.01, t_to=30.01, dt=0.05, margin=0.5, max_delay_steps=150)
    rng = np.random.RandomState(3)
    tracks = []
    for k in range(40):
        W = 1 + k % 9
        t = np.cumsum(rng.uniform(0.3, 2.0, W)) + rng.uniform(-6.0, 20.0)
        a, b = s.starts[k % N][:2], s.goals[(k * 7) % N][:2]
        lam = np.linspace(0.0, 1.0, W)[:, None]
        tracks.append(((0.0, 0.3, 1.0)[k % 3], np.column_stack([t, a + lam * (b - a)])))
    grown, grown_tracks = s.pipe.deconflict_tracks(s.all_tickets, t_start, tracks, pairs=[], **kw)
    assert s.pipe.in_flight() == 8
    drain(s.pipe, 8)
    s.pipe.release(flying)
    idle, idle_tracks = s.pipe.deconflict_tracks(s.all_tickets, t_start, tracks, pairs=[], **kw)
    assert grown.tobytes() == idle.tobytes() and grown_tracks.tobytes() == idle_tracks.tobytes() and grown_tracks.shape == (N + 2, 40)
    assert (grown.blocker >= N + 2).sum() >= 3 and (grown_tracks.status == 1).any() and (grown_tracks.status == 2).any()
    # deconflict() afterwards, in the buffers this call has grown, is what it is without it
    look = dict(t_from=0.0, t_to=12.95, dt=0.1, margin=0.5, max_delay_steps=10)
    a = s.pipe.deconflict(s.tickets[:12], t_start[:12], **look)
    s.pipe.deconflict_tracks(s.tickets[:5], t_start[:5], small, **look)
    assert s.pipe.deconflict(s.tickets[:12], t_start[:12], **look).tobytes() == a.tobytes()


def test_refusals_launch_nothing_and_leave_the_pipeline_usable():
    """every refusal of the track set, and the delay call's, are PP_ERR_INVALID with the first offender named; a valid call afterwards gives the records
    of before"""
    from pathplanning_amd._lib import ConflictParams, DelayParams, DelayResult, PPError, TrackResult, TrackSet, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    pipe.speed_profile(held[:8], samples=False)
    tracks = [(0.3, [(0.0, 1.0, 1.0), (1.0, 2.0, 2.0)]), (1.0, [(5.0, 0.0, 0.0)]), (0.0, [(-1.0, 3.0, 3.0), (0.0, 3.0, 4.0), (0.5, -3.0, 4.0)])]
    call = dict(t_to=10.0, margin=0.5, max_delay_steps=30)
    first, first_tracks = pipe.deconflict_tracks(held[:6], np.arange(6.0) * 0.1, tracks, **call)
    out, rec = (DelayResult * 128)(), (TrackResult * 512)()
    good = dict(t_from=0.0, t_to=10.0, dt=0.1, margin=0.5, hold_before=0, hold_after=0, max_delay_steps=30, reserved=0)
    offsets = np.array([0, 2, 3, 6], dtype=np.int32)
    waypoints = np.concatenate([np.asarray(w, dtype=np.float64) for _, w in tracks])
    radii = np.array([0.3, 1.0, 0.0])

    def refused(*words, tickets=held[:2], ts=0.0, n_pairs=None, params=good, M=3, reserved=0, o=offsets, w=waypoints, r=radii):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        ts = None if ts is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ts, dtype=np.float64), (len(t),)))
        np_ = len(t) * (len(t) - 1) // 2 if n_pairs is None else n_pairs
        dp = DelayParams(ConflictParams(*[params[k] for k in ("t_from", "t_to", "dt", "margin", "hold_before", "hold_after")]), params["max_delay_steps"], params["reserved"])
        keep = [None if a is None else np.ascontiguousarray(a) for a in (o, w, r)]
        tk = TrackSet(M, reserved, *(None if a is None else a.ctypes.data for a in keep))
        rc = lib.pp_pipeline_deconflict_tracks(pipe.h, len(t), ptr(t), ptr(ts), np_, None, C.byref(dp), C.byref(tk), out, rec)
        msg = lib.pp_last_error().decode()
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    # the track set's
    refused("track set", "reserved", reserved=1)
    refused("n_tracks", "-1", M=-1)
    refused("n_tracks", "65537", M=(1 << 16) + 1)
    refused("null offsets", o=None)
    refused("null waypoints", w=None)
    refused("null radii", r=None)
    refused("offsets[0]", o=np.array([1, 2, 3, 6], dtype=np.int32))
    refused("track 1", "no waypoint", o=np.array([0, 2, 2, 6], dtype=np.int32))
    refused("track 2", "strictly increasing", o=np.array([0, 2, 3, 1], dtype=np.int32))
    refused("16777217", "waypoints", M=1, o=np.array([0, (1 << 24) + 1], dtype=np.int32))
    many = 1 << 16  # 2^16 tracks of one waypoint on 1025 lattice times: one sample more than 2^26
    refused("track samples", str(many * 1025), M=many, o=np.arange(many + 1, dtype=np.int32), w=np.zeros((many, 3)), r=np.zeros(many), params=dict(good, t_to=102.4 + 1e-6))
    for bad in (float("nan"), float("inf"), -float("inf")):
        for c in range(3):
            w = waypoints.copy()
            w[4, c] = bad
            refused("waypoint 4 of track 2", "not finite", w=w)
        refused("track 1", "radius", r=np.array([0.3, bad, 0.0]))
    refused("track 2", "radius", r=np.array([0.3, 1.0, -1e-3]))
    w = waypoints.copy()
    w[1, 0] = w[0, 0]
    refused("waypoint 1 of track 0", "strictly increasing", w=w)
    w = waypoints.copy()
    w[5, 0] = -0.25
    refused("waypoint 5 of track 2", "strictly increasing", w=w)
    # the delay call's and the conflict call's come first
    refused("max_delay_steps", ">= 0", params=dict(good, max_delay_steps=-1), reserved=1)
    refused("reserved", "delay call", params=dict(good, reserved=1))
    refused("T + max_delay_steps", params=dict(good, max_delay_steps=(1 << 20) - 100))
    refused("capacity", tickets=(held + held)[:CAPACITY + 1])
    refused("ticket %d" % 10 ** 9, "unknown", tickets=[held[0], 10 ** 9])
    refused("ticket %d" % held[3], "twice", tickets=[held[3], held[4], held[3]])
    refused("ticket %d" % held[9], "speed_profile first", tickets=[held[0], held[9]])
    refused("t_start", ts=None)
    refused("ticket %d" % held[1], "t_start", tickets=held[:3], ts=[0.0, float("nan"), 1.0])
    refused("dt", "> 0", params=dict(good, dt=0.0))
    refused("margin", ">= 0", params=dict(good, margin=-0.01))
    refused("n_pairs", n_pairs=-1, tickets=held[:3])
    refused("n (n - 1) / 2 = 3", n_pairs=2, tickets=held[:3])
    # the batch entry on the pipeline's buffer set
    dp = DelayParams(ConflictParams(0.0, 10.0, 0.1, 0.5, 0, 0), 30, 0)
    rc = lib.pp_planner_deconflict_tracks(pipe.planner_h, 1, ptr(np.zeros(1)), 0, None, C.byref(dp), None, out, rec)
    assert rc == PP_ERR_INVALID and "pp_pipeline_deconflict_tracks" in lib.pp_last_error().decode()
    # the wrapper: PPError from the library, ValueError for what it cannot lay out
    with pytest.raises(PPError) as e:
        pipe.deconflict_tracks(held[:2], [0.0, 0.0], [(-1.0, [(0.0, 0.0, 0.0)])])
    assert e.value.code == PP_ERR_INVALID and "track 0" in str(e.value) and "radius" in str(e.value)
    with pytest.raises(ValueError):
        pipe.deconflict_tracks(held[:2], [0.0, 0.0], [(1.0, np.zeros((0, 3)))])
    with pytest.raises(ValueError):
        pipe.deconflict_tracks(held[:2], [0.0, 0.0], [(1.0, np.zeros((2, 2)))])
    # everything is as it was
    again, again_tracks = pipe.deconflict_tracks(held[:6], np.arange(6.0) * 0.1, tracks, **call)
    assert again.tobytes() == first.tobytes() and again_tracks.tobytes() == first_tracks.tobytes()


def test_the_batch_form_equals_the_pipeline_form():
    """HybridAStarBatch.deconflict_tracks: the same kernels with identity slots on the same queries give the same records, field by field"""
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
        batch.deconflict_tracks(np.zeros(n), None, max_delay_steps=5)
    assert e.value.code == PP_ERR_INVALID and "query 0" in str(e.value) and "speed_profile first" in str(e.value)
    which, pairs, t_start, discs, kw, tickets, recs, rows, tracks = call_of(f, "chain")
    assert list(which) == list(range(n))
    _, rows = batch.speed_profile(**LIM)
    for pr in (pairs, None, []):
        mine, mine_tracks = batch.deconflict_tracks(t_start, tracks, pairs=pr, **kw)
        theirs, their_tracks = s.pipe.deconflict_tracks(tickets, t_start, tracks, pairs=pr, **kw)
        for name in mine.dtype.names:
            assert np.array_equal(mine[name], theirs[name]), name
        assert mine.tobytes() == theirs.tobytes() and mine_tracks.tobytes() == their_tracks.tobytes() and mine_tracks.shape == (n, len(tracks))
        _, _, want, want_tracks = restate(f, range(n), rows, t_start, pr, s.point, tracks, **kw)
        compare(mine, mine_tracks, want, want_tracks, "batch form")
    some, some_tracks = batch.deconflict_tracks(t_start[:5], tracks, 5, pairs=[(4, 0), (2, 3)], **kw)
    assert len(some) == 5 and some_tracks.shape == (5, len(tracks))
    batch.close()


def test_the_cpp_mirror_finds_the_delays_of_a_plain_sequential_loop():
    """tests/cpp/test_pipeline_deconflict_tracks.cpp: DeconflictTracks(tickets, starts, tracks) of Planner::HybridAStarPipeline against a loop over the
    device's own poses and the tracks' waypoints"""
    import os
    import subprocess
    from pathplanning_amd import build
    exe = build.build_pipeline_deconflict_tracks_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"DeconflictTracks(tickets, starts, tracks) == the sequential loop over the device's poses" in r.stdout
