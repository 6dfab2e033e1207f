"""-m gpu: the pairs of held plans that can meet, by a space-time broad phase (pp_pipeline_candidate_pairs, pp_planner_candidate_pairs; k_plan_boxes,
k_box_pairs and k_pair_offsets in pathplanning_amd/csrc/pp_pairs.hpp; the definition is in include/pp_hip.h).

The comparator is tests/pair_restatement.py, a restatement in numpy that shares nothing with the kernels, fed the device's OWN extended trajectory:
the poses of conflicts(poses=True) over the horizon that begins max_delay_steps lattice steps earlier.  A box is a min and a max of those doubles and
the rule is one subtraction and one comparison per axis and direction, so NOTHING is excluded: the boxes are equal bit for bit (NaNs included) and
the pair list, first_box, n_found, n_boxed, n_boxes and reach are EQUAL.  Independent of any restatement: every pair the conflict call finds in
conflict is listed, and the delay calls give the same bytes over the list as over every pair.

Scene: the one of tests/test_gpu_pipeline_stamp.py (48 plans held in a capacity-64 pipeline, shared with the other files of that scene), and a batch
planner over 130 queries of the same world and recipe for rows with more than one wave of partners.  Every test leaves the pipeline without a
footprint and with nothing in flight."""
import ctypes as C
import functools

import numpy as np
import pytest

import conflict_restatement as CR
import pair_restatement as PR
from test_conflict_restatement_host import LIM, starts_of
from test_delay_restatement_host import HOLDS, cases
from test_gpu_pipeline_conflicts import bits, fleet
from test_gpu_pipeline_stamp import CAPACITY, N, _queries, drain

pytestmark = pytest.mark.gpu

PP_ERR_INVALID = -1
NAMES = ["T=1", "T=63", "T=64", "T=65", "D=0", "D=1", "D=65"] + ["nearest, " + h for h in HOLDS] + ["CAR3"]


def split(kw):
    """(the lattice keywords of a case, its largest delay)"""
    return {k: v for k, v in kw.items() if k != "max_delay_steps"}, int(kw["max_delay_steps"])


def own_poses(holder, who, t_start, look, D):
    """the device's own extended trajectory, [n, T + D, 3] with NaN where absent, and T: the poses of a conflict call whose horizon begins D lattice steps
    (and half a step) earlier; `who` is (tickets,) for a pipeline and () for a batch planner"""
    k0, T = CR.lattice(look["t_from"], look["t_to"], look["dt"])
    wider = dict(look, t_from=(k0 - D - 0.5) * look["dt"])
    assert CR.lattice(wider["t_from"], wider["t_to"], wider["dt"]) == (k0 - D, T + D)
    poses = np.array(holder.conflicts(*who, t_start, pairs=[(0, 1)], poses=True, **wider)[2], dtype=np.float64)
    assert poses.shape == (len(t_start), T + D, 3)
    return poses, T


def same(got, want, what):
    """a call's (pairs, first_box, summary, boxes) against the restatement's dict: everything EQUAL"""
    pairs, first, summary, boxes = got
    assert boxes.shape == want["boxes"].shape and np.array_equal(np.isnan(boxes), np.isnan(want["boxes"])), what
    there = ~np.isnan(boxes)
    assert np.array_equal(bits(boxes[there]), bits(want["boxes"][there])), what
    assert np.isnan(boxes).all(axis=2)[np.isnan(boxes[:, :, 0])].all()  # (a box that is not there is four NaNs)
    assert (summary.n_found, summary.n_written, summary.n_boxes, summary.n_boxed, summary.reserved) == (want["n_found"], want["n_found"], want["n_boxes"], want["n_boxed"], 0), (
        what, summary.n_found, summary.n_boxed, want["n_found"], want["n_boxed"])
    assert bits(summary.reach) == bits(want["reach"]), (what, summary.reach, want["reach"])
    assert pairs.dtype == np.int32 and first.dtype == np.int32 and pairs.shape == (want["n_found"], 2) and first.shape == (want["n_found"],), what
    assert np.array_equal(pairs, want["pairs"]) and np.array_equal(first, want["first_box"]), what


class with_footprint:
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


def case_of(f, name):
    which, _, t_start, discs, kw = cases(f.s.starts)[name]
    tickets = f.s.tickets[which]
    recs = f.s.pipe.speed_profile(tickets, samples=False, **LIM)
    recs = recs[0] if isinstance(recs, tuple) else recs
    look, D = split(kw)
    return which, t_start, discs, look, D, tickets, recs


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_exact_on_the_devices_own_poses(name):
    """lattices of 1, 63, 64, 65 and 130 times, largest delays of 0, 1, 64 and 65 steps, all 48 plans (a failed query among them: never listed) under the
    four combinations of the hold flags, and a three-disc footprint; each at 1, 16, 64 and T lattice times per box"""
    f = fleet()
    s = f.s
    which, t_start, discs, look, D, tickets, recs = case_of(f, name)
    n = len(which)
    with with_footprint(s, discs if name == "CAR3" else None):
        poses, T = own_poses(s.pipe, (tickets,), t_start, look, D)
        for B in sorted({1, 16, 64, T}):
            got = s.pipe.candidate_pairs(tickets, t_start, times_per_box=B, max_delay_steps=D, boxes=True, **look)
            want = PR.candidate_pairs(poses, T, D, B, discs, look["margin"])
            same(got, want, (name, B))
            print("%s, B = %d: %d of %d pairs, %d boxes, %d plans boxed" % (name, B, len(got[0]), n * (n - 1) // 2, got[2].n_boxes, got[2].n_boxed))
            assert 0 < len(got[0]) < n * (n - 1) // 2
            keys = got[0][:, 0].astype(np.int64) * n + got[0][:, 1]
            assert (got[0][:, 0] < got[0][:, 1]).all() and (np.diff(keys) > 0).all()  # strictly ascending in (i, j)
            again = s.pipe.candidate_pairs(tickets, t_start, times_per_box=B, max_delay_steps=D, boxes=True, **look)
            assert all(a.tobytes() == b.tobytes() for a, b in zip((got[0], got[1], got[3]), (again[0], again[1], again[3]))) and bytes(got[2]) == bytes(again[2])
    if name.startswith("nearest"):
        failed = [q for q in range(N) if recs[q].status != 0]
        assert failed and not np.isin(got[0], failed).any() and np.isnan(got[3][failed]).all() and got[2].n_boxed <= N - len(failed)


@functools.lru_cache(maxsize=None)
def batch_of_130():
    """130 queries of the scene's world and recipe in a batch planner, profiled: row 0 of the pair matrix has 129 partners, two full chunks of 64 lanes
    and a tail of one"""
    import pathplanning_amd as pa
    s = fleet().s
    starts, goals, seeds = _queries(s.w, 130)
    batch = pa.HybridAStarBatch(s.val, max_batch=130, max_nodes=32768)
    batch.initialize(s.pipe.nonholo_table())
    res = batch.search_batch(starts, goals, seeds)
    assert sum(r.status == 0 for r in res) >= 100
    batch.speed_profile(samples=False, **LIM)
    return batch


@pytest.mark.parametrize("D", [0, 65])
def test_more_than_one_wave_of_partners_in_the_batch_form(D):
    batch = batch_of_130()
    s = fleet().s
    t_start = starts_of(130)
    look = dict(t_from=0.7 - 1e-9, t_to=0.1 * (7 + 130 - 1) + 0.05, dt=0.1, margin=0.5)
    poses, T = own_poses(batch, (), t_start, look, D)
    assert T == 130
    for B in (16, T):
        got = batch.candidate_pairs(t_start, times_per_box=B, max_delay_steps=D, boxes=True, **look)
        want = PR.candidate_pairs(poses, T, D, B, s.point, look["margin"])
        same(got, want, ("batch of 130", D, B))
        pairs = got[0]
        print("batch of 130, D = %d, B = %d: %d of %d pairs" % (D, B, len(pairs), 130 * 129 // 2))
        assert 0 < len(pairs) < 130 * 129 // 2
        # some row among the first three (one of them may be a failed query) has partners in its first and in its second chunk of 64 lanes
        chunk = (pairs[:, 1] - pairs[:, 0] - 1) // 64
        assert any({0, 1} <= set(chunk[pairs[:, 0] == i].tolist()) for i in range(3))
        if B == T and D == 65:
            assert len(pairs) > max(1024, 8 * 130)  # (the wrapper's first buffer was outgrown: it called again)
    some = batch.candidate_pairs(t_start[:70], 70, times_per_box=16, max_delay_steps=D, **look)
    inside = PR.candidate_pairs(poses[:70], T, D, 16, s.point, look["margin"])
    assert np.array_equal(some[0], inside["pairs"]) and np.array_equal(some[1], inside["first_box"]) and some[2].n_found == inside["n_found"]
    # more boxes than a call may form: 130 plans with a box per lattice time of a horizon of 1048571 times
    from pathplanning_amd._lib import PPError
    with pytest.raises(PPError) as e:
        batch.candidate_pairs(t_start, times_per_box=1, t_from=0.0, t_to=104857.0, dt=0.1)
    assert e.value.code == PP_ERR_INVALID and "n * NB" in str(e.value)
    assert np.array_equal(batch.candidate_pairs(t_start[:70], 70, times_per_box=16, max_delay_steps=D, **look)[0], some[0])


@pytest.mark.parametrize("name", ["D=0", "nearest, absent", "nearest, hold-both", "CAR3"])
def test_every_pair_the_conflict_call_finds_in_conflict_is_listed(name):
    """independent of any restatement, D = 0: conflicts(pairs=None) over the same lattice; every pair with status 1 is in the list, for every B"""
    f = fleet()
    s = f.s
    which, t_start, discs, look, _, tickets, _ = case_of(f, name)
    n = len(which)
    with with_footprint(s, discs if name == "CAR3" else None):
        found = s.pipe.conflicts(tickets, t_start, **look)[1]
        hit = {p for p, r in zip(CR.all_pairs(n), found) if r.status == 1}
        assert len(hit) >= 1
        T = CR.lattice(look["t_from"], look["t_to"], look["dt"])[1]
        for B in sorted({1, 16, 64, T}):
            pairs = s.pipe.candidate_pairs(tickets, t_start, times_per_box=B, max_delay_steps=0, **look)[0]
            listed = {(int(a), int(b)) for a, b in pairs}
            assert hit <= listed and len(listed) < n * (n - 1) // 2, (name, B, hit - listed)
        # the conflict call over the list: the records of the listed pairs, byte for byte
        some = s.pipe.conflicts(tickets, t_start, pairs=pairs, **look)[1]
        index = {p: k for k, p in enumerate(CR.all_pairs(n))}
        assert all(bytes(r) == bytes(found[index[(int(a), int(b))]]) for r, (a, b) in zip(some, pairs))


@pytest.mark.parametrize("name", ["all-12", "D=64", "CAR3", "nearest, absent"])
def test_the_delay_call_over_the_list_gives_the_bytes_of_the_call_over_every_pair(name):
    f = fleet()
    s = f.s
    which, t_start, discs, look, D, tickets, _ = case_of(f, name)
    with with_footprint(s, discs if name == "CAR3" else None):
        every = s.pipe.deconflict(tickets, t_start, pairs=None, max_delay_steps=D, **look)
        for B in (16, 64):
            pairs = s.pipe.candidate_pairs(tickets, t_start, times_per_box=B, max_delay_steps=D, **look)[0]
            assert s.pipe.deconflict(tickets, t_start, pairs=pairs, max_delay_steps=D, **look).tobytes() == every.tobytes(), (name, B)
    assert (every.delay_steps > 0).any() or name == "D=0"


def test_the_delay_call_with_tracks_over_the_list_gives_the_bytes_of_the_call_over_every_pair():
    from test_gpu_pipeline_deconflict_tracks import call_of
    f = fleet()
    s = f.s
    which, _, t_start, discs, kw, tickets, recs, rows, tracks = call_of(f, "chain")
    look, D = split(kw)
    every, every_tracks = s.pipe.deconflict_tracks(tickets, t_start, tracks, pairs=None, **kw)
    pairs = s.pipe.candidate_pairs(tickets, t_start, times_per_box=16, max_delay_steps=D, **look)[0]
    got, got_tracks = s.pipe.deconflict_tracks(tickets, t_start, tracks, pairs=pairs, **kw)
    assert 0 < len(pairs) < 120 and got.tobytes() == every.tobytes() and got_tracks.tobytes() == every_tracks.tobytes()
    assert (every.blocker >= 0).any()


def test_truncation_writes_the_head_of_the_list_and_nothing_behind_it():
    from pathplanning_amd._lib import ConflictParams, DelayParams, PairParams, PairSummary, ptr
    f = fleet()
    s = f.s
    which, t_start, discs, look, D, tickets, _ = case_of(f, "nearest, absent")
    full, first, summary = s.pipe.candidate_pairs(tickets, t_start, times_per_box=16, max_delay_steps=D, **look)
    found = int(summary.n_found)
    assert found == len(full) > 100
    t = np.ascontiguousarray(tickets, dtype=np.uint64)
    ts = np.ascontiguousarray(t_start, dtype=np.float64)
    cp = ConflictParams(look["t_from"], look["t_to"], look["dt"], look["margin"], int(look.get("hold_before", False)), int(look.get("hold_after", False)))
    for room in (0, 1, found - 1, found):
        head, box, sm = s.pipe.candidate_pairs(tickets, t_start, times_per_box=16, max_delay_steps=D, max_pairs=room, **look)
        assert (sm.n_found, sm.n_written) == (found, room) and np.array_equal(head, full[:room]) and np.array_equal(box, first[:room])
        # through the C ABI, into arrays with a guard behind the caller's rows
        pairs, boxes, out = np.full((found + 8, 2), -7, dtype=np.int32), np.full(found + 8, -7, dtype=np.int32), PairSummary()
        pp = PairParams(DelayParams(cp, D, 0), 16, room)
        assert s.pipe.lib.pp_pipeline_candidate_pairs(s.pipe.h, len(t), ptr(t), ptr(ts), C.byref(pp), ptr(pairs), ptr(boxes), None, C.byref(out)) == 0
        assert (out.n_found, out.n_written) == (found, room) and np.array_equal(pairs[:room], full[:room]) and np.array_equal(boxes[:room], first[:room])
        assert (pairs[room:] == -7).all() and (boxes[room:] == -7).all()
    # more room than pairs; no first_box, no summary; no pairs_host with max_pairs == 0
    pp = PairParams(DelayParams(cp, D, 0), 16, found + 8)
    pairs = np.full((found + 8, 2), -7, dtype=np.int32)
    assert s.pipe.lib.pp_pipeline_candidate_pairs(s.pipe.h, len(t), ptr(t), ptr(ts), C.byref(pp), ptr(pairs), None, None, None) == 0
    assert np.array_equal(pairs[:found], full) and (pairs[found:] == -7).all()
    pp = PairParams(DelayParams(cp, D, 0), 16, 0)
    out = PairSummary()
    assert s.pipe.lib.pp_pipeline_candidate_pairs(s.pipe.h, len(t), ptr(t), ptr(ts), C.byref(pp), None, None, None, C.byref(out)) == 0 and (out.n_found, out.n_written) == (found, 0)
    small = s.pipe.candidate_pairs(tickets, t_start, times_per_box=16, max_delay_steps=D, max_pairs=5, **look)
    assert len(small[0]) == 5 and small[2].n_found == found


def test_no_plan_one_plan_and_the_refusals_leave_the_pipeline_usable():
    """every refusal is PP_ERR_INVALID with nothing launched; a valid call afterwards gives the bytes of before; n == 0 and n == 1 are PP_OK with an empty list"""
    from pathplanning_amd._lib import ConflictParams, DelayParams, PairParams, PairSummary, PPError, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    pipe.speed_profile(held[:8], samples=False)
    kw = dict(t_from=0.0, t_to=10.0, dt=0.1, margin=0.5)
    first = pipe.candidate_pairs(held[:6], np.arange(6.0) * 0.1, times_per_box=16, max_delay_steps=30, boxes=True, **kw)
    good = dict(kw, hold_before=0, hold_after=0, max_delay_steps=30, reserved=0, times_per_box=16, max_pairs=64)
    pairs, boxes, out = np.zeros((128, 2), dtype=np.int32), np.zeros(128, dtype=np.int32), PairSummary()

    def call(tickets, n=None, ts=0.0, params=good, pairs_host=pairs):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        count = len(t) if n is None else n
        ts = None if ts is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ts, dtype=np.float64), (len(t),)))
        pp = None
        if params is not None:
            cp = ConflictParams(*[params[k] for k in ("t_from", "t_to", "dt", "margin", "hold_before", "hold_after")])
            pp = PairParams(DelayParams(cp, params["max_delay_steps"], params["reserved"]), params["times_per_box"], params["max_pairs"])
        rc = lib.pp_pipeline_candidate_pairs(pipe.h, count, ptr(t), ptr(ts), C.byref(pp) if pp is not None else None, ptr(pairs_host), ptr(boxes), None, C.byref(out))
        return rc, lib.pp_last_error().decode()

    def refused(tickets, *words, **how):
        rc, msg = call(tickets, **how)
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    # the call's own
    for bad in (0, -1, (1 << 20) + 1):
        refused(held[:2], "times_per_box", params=dict(good, times_per_box=bad))
    refused(held[:2], "max_pairs", ">= 0", params=dict(good, max_pairs=-1))
    refused(held[:2], "null pairs_host", pairs_host=None)
    # (n * NB > 2^26 needs more than 64 plans: the batch form's test refuses it)
    refused(held[:2], "reserved", params=dict(good, reserved=1))
    # the delay call's
    refused(held[:2], "max_delay_steps", ">= 0", params=dict(good, max_delay_steps=-1))
    refused(held[:2], "T + max_delay_steps", params=dict(good, max_delay_steps=(1 << 20) - 100))
    refused((held + held)[:CAPACITY + 1], "capacity")
    refused(held[:1], "capacity", n=-1)
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused([held[0], held[9]], "ticket %d" % held[9], "speed_profile first")  # held, but not in the last speed-profile call
    refused(held[:2], "t_start", ts=None)
    refused(held[:2], "params", params=None)
    for bad in (float("nan"), float("inf")):
        refused(held[:3], "ticket %d" % held[1], "t_start", ts=[0.0, bad, 1.0])
        refused(held[:2], "t_from", params=dict(good, t_from=bad))
    refused(held[:2], "t_from <= t_to", params=dict(good, t_from=2.0, t_to=1.0))
    for bad in (0.0, -0.1, float("nan")):
        refused(held[:2], "dt", "> 0", params=dict(good, dt=bad))
    for bad in (-0.01, float("nan")):
        refused(held[:2], "margin", ">= 0", params=dict(good, margin=bad))
    refused(held[:2], "lattice times", "no", params=dict(good, t_from=0.55, t_to=0.55, dt=0.25))
    refused(held[:2], "lattice times", "more than", params=dict(good, dt=1e-300))
    refused(held[:2], "hold_before and hold_after", params=dict(good, hold_after=2))
    # the batch entry on the pipeline's buffer set
    pp = PairParams(DelayParams(ConflictParams(0.0, 10.0, 0.1, 0.5, 0, 0), 30, 0), 16, 64)
    rc = lib.pp_planner_candidate_pairs(pipe.planner_h, 1, ptr(np.zeros(1)), C.byref(pp), ptr(pairs), None, None, None)
    assert rc == PP_ERR_INVALID and "pp_pipeline_candidate_pairs" in lib.pp_last_error().decode()
    # in flight: refused; released since the profile, by either route: refused, and the rest answers as before
    flying = [int(t) for t in pipe.submit(s.goals[8:10], s.starts[8:10], np.array([944, 945], dtype=np.uint64))]
    assert len(flying) == 2 and pipe.in_flight() == 2
    refused([held[0], flying[0]], "ticket %d" % flying[0], "in flight")
    res = drain(pipe, 2)
    refused([held[0], flying[0]], "ticket %d" % flying[0], "speed_profile first")
    pipe.speed_profile([held[0], held[1]] + flying, samples=False)
    with_them = pipe.candidate_pairs([held[0], held[1]] + flying, [0.0, 0.1, 0.0, 0.0], times_per_box=16, max_delay_steps=30, **kw)
    assert with_them[2].n_boxes == 7 and with_them[2].n_found == len(with_them[0]) <= 6
    free = pipe.free_slots()
    pipe.release(flying[:1])
    if res[flying[1]].status == 0:
        pipe.get_paths(flying[1:], max_poses=64, release=True)
    else:
        pipe.release(flying[1:])
    assert pipe.free_slots() == free + 2
    for t in flying:
        refused([held[0], t], "ticket %d" % t, "released")
        with pytest.raises(PPError) as e:
            pipe.candidate_pairs([t], [0.0])
        assert e.value.code == PP_ERR_INVALID and "ticket %d" % t in str(e.value)
    with pytest.raises(PPError):
        pipe.candidate_pairs(held[:2], [0.0, 0.0], times_per_box=0)
    with pytest.raises(ValueError):
        pipe.candidate_pairs(held[:3], [1.0, 2.0])
    with pytest.raises(TypeError):
        pipe.candidate_pairs(held[:2], [1.0, 2.0], pairs=None)
    # n == 0 and n == 1
    assert lib.pp_pipeline_candidate_pairs(pipe.h, 0, None, None, None, None, None, None, None) == 0
    out.n_found = 5
    assert lib.pp_pipeline_candidate_pairs(pipe.h, 0, None, None, None, None, None, None, C.byref(out)) == 0 and bytes(out) == bytes(32)
    none = pipe.candidate_pairs([], [])
    assert none[0].shape == (0, 2) and none[1].shape == (0,) and none[2].n_found == 0
    one = pipe.candidate_pairs(held[:1], [0.0], times_per_box=16, boxes=True, **kw)
    assert one[0].shape == (0, 2) and (one[2].n_found, one[2].n_written, one[2].n_boxes) == (0, 0, 7) and one[3].shape == (1, 7, 4)
    assert one[2].n_boxed == int(not np.isnan(one[3]).all())
    # everything is as it was (the profile of the first eight is gone: the last speed-profile call replaced it)
    refused(held[:6], "ticket %d" % held[2], "speed_profile first")
    pipe.speed_profile(held[:8], samples=False)
    again = pipe.candidate_pairs(held[:6], np.arange(6.0) * 0.1, times_per_box=16, max_delay_steps=30, boxes=True, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((first[0], first[1], first[3]), (again[0], again[1], again[3]))) and bytes(first[2]) == bytes(again[2])


def test_beside_eight_queries_in_flight_the_buffers_grow_and_the_list_is_the_idle_calls():
    """a small n x NB, then more plans, more boxes and more pairs than any call before, with eight queries in flight: every buffer of the service grows
    and the outgrown ones are parked; the call reads no map and the list equals the idle call's"""
    f = fleet()
    s = f.s
    s.pipe.speed_profile(s.all_tickets, samples=False, **LIM)
    t_start = np.concatenate([starts_of(N), [0.0, 2.0]])
    s.pipe.candidate_pairs(s.all_tickets[:2], t_start[:2], t_to=1.0, times_per_box=64)
    flying = s.pipe.submit(s.goals[8:16], s.starts[8:16], np.arange(980, 988, dtype=np.uint64))
    assert len(flying) == 8 and s.pipe.in_flight() == 8
    kw = dict(t_from=-5.01, t_to=30.01, dt=0.05, margin=0.5, times_per_box=2, max_delay_steps=150, boxes=True)
    small = s.pipe.candidate_pairs(s.all_tickets[:5], t_start[:5], **kw)
    grown = s.pipe.candidate_pairs(s.all_tickets, t_start, **kw)
    assert s.pipe.in_flight() == 8
    drain(s.pipe, 8)
    s.pipe.release(flying)
    for got, who in ((small, slice(0, 5)), (grown, slice(None))):
        idle = s.pipe.candidate_pairs(s.all_tickets[who], t_start[who], **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((got[0], got[1], got[3]), (idle[0], idle[1], idle[3]))) and bytes(got[2]) == bytes(idle[2])
    assert grown[2].n_boxes == 351 and len(grown[0]) > 100 and grown[3].shape == (N + 2, 351, 4)
    # a delay call afterwards, in the trajectory buffers the broad phase has grown, is what it is without one
    look = dict(t_from=0.0, t_to=12.95, dt=0.1, margin=0.5)
    a = s.pipe.deconflict(s.tickets, t_start[:N], pairs=grown[0][(grown[0] < N).all(axis=1)], max_delay_steps=20, **look)
    s.pipe.candidate_pairs(s.tickets[:5], t_start[:5], times_per_box=3, max_delay_steps=2, **look)
    b = s.pipe.deconflict(s.tickets, t_start[:N], pairs=grown[0][(grown[0] < N).all(axis=1)], max_delay_steps=20, **look)
    assert a.tobytes() == b.tobytes()


def test_the_cpp_mirror_lists_the_pairs_of_a_plain_sequential_loop():
    """tests/cpp/test_pipeline_candidate_pairs.cpp: CandidatePairs(tickets, starts) of Planner::HybridAStarPipeline against a loop over the device's own poses"""
    import os
    import subprocess
    from pathplanning_amd import build
    exe = build.build_pipeline_candidate_pairs_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"CandidatePairs(tickets, starts) == the sequential loop over the device's poses" in r.stdout
