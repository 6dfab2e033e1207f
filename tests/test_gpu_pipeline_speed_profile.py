"""-m gpu: speed profiles and arrival times along held plans, by ticket (pp_pipeline_speed_profile, pp_planner_speed_profile;
k_speed_profile_tickets in pathplanning_amd/csrc/pp_speed_profile.hpp; the definition is in include/pp_hip.h).

The comparator is tests/speed_restatement.py, a restatement in numpy that shares nothing with the kernel; the plans' edges are rebuilt from
get_path_of as tests/test_gpu_pipeline_locate.py rebuilds them.  On every plan status, n_samples, n_cusps and length are EQUAL (length to
revalidate's) and s is EQUAL bit for bit.  v is EQUAL bit for bit at every DECIDED sample (its Reeds-Shepp sample more than 1e-9 m from a boundary
between two motions and, with the clearance term, every disc centre more than 1e-9 m from a cell border) and within 1e-12 relative at the others; at
most footprint_ref.MAX_LEFT_OUT of the samples of a comparison of 1000 samples or more, and of all samples this file compares, may be undecided (tests/test_speed_restatement_host.py checks on the CPU that the
restatement alone stays within that on the oracle's plans of the same queries).  t and the duration agree within 1e-9 relative, a bound that holds
for any order of summation: at most 2^20 additions of relative error 2^-53 each is about 1.2e-10, so 1e-9 leaves a margin of roughly eight (the kernel
sums in sample order, as the definition does).  t never decreases along a plan.

Scene: the one of tests/test_gpu_pipeline_stamp.py (synthetic_world(256, 14, 3), validator (1.0, 0.1), 48 plans held in a capacity-64 pipeline, shared
with that file when both run in one process).  Every test leaves the pipeline without a footprint and with nothing in flight."""
import ctypes as C
import functools
import math
import os
import subprocess
import time

import numpy as np
import pytest

import footprint_ref as FR
import locate_restatement as R
import oracle_lib as O
import speed_restatement as V
from test_gpu_pipeline_locate import restated
from test_gpu_pipeline_stamp import CAPACITY, N, Plans, _world, drain, scene
from test_locate_restatement_host import cusp_of

pytestmark = pytest.mark.gpu

PP_ERR_INVALID = -1
T_TOL = 1e-9
V_TOL = 1e-12
ZERO_FIELDS = ("n_cusps", "reserved", "s_first", "s_last", "duration", "v_peak", "min_clearance", "s_min_clearance")
POINT = [(0.0, 0.0, 1.0)]  # the point validator of the scene's maps (min_safe_radius 1.0) seen as a disc


TOTAL = [0, 0]  # samples compared by this file so far, and how many of them were undecided


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def close(a, b, tol):
    return np.abs(np.asarray(a) - np.asarray(b)) <= tol * np.abs(np.asarray(b))


def compare(recs, rows, want, what, lengths=None):
    """the records and (s, v, t) rows of the device against the restatement's, plan by plan; returns (samples, undecided samples)"""
    assert len(recs) == len(want) and (rows is None or len(rows) == len(want))
    samples = undecided = 0
    for i, (a, b) in enumerate(zip(recs, want)):
        print("%s plan %3d: status %d samples %d cusps %d length %.17g first %.17g last %.17g duration %.17g peak %.17g clearance %.9g at %.17g | want status %d samples %d cusps %d duration %.17g" %
              (what, i, a.status, a.n_samples, a.n_cusps, a.length, a.s_first, a.s_last, a.duration, a.v_peak, a.min_clearance, a.s_min_clearance, b["status"], b["n_samples"],
               b["n_cusps"], b["duration"]))
        assert (a.status, a.n_samples, a.n_cusps) == (b["status"], b["n_samples"], b["n_cusps"]) and a.length == b["length"], (what, i)
        if lengths is not None:
            assert a.length == lengths[i], (what, i)
        if b["status"] != 0:
            assert all(getattr(a, f) == 0 for f in ZERO_FIELDS), (what, i)
            assert rows is None or len(rows[i]) == 0
            continue
        left = int((~b["decided"]).sum())
        samples += b["n_samples"]
        undecided += left
        if rows is not None:
            s, v, t = rows[i][:, 0], rows[i][:, 1], rows[i][:, 2]
            assert np.array_equal(bits(s), bits(b["s"])), (what, i, "s")
            same = bits(v) == bits(b["v"])
            if not (same | ~b["decided"]).all():
                k = int(np.flatnonzero(~same & b["decided"])[0])
                raise AssertionError((what, i, "v at decided sample", k, float(v[k]), float(b["v"][k])))
            assert close(v, b["v"], V_TOL).all(), (what, i, "v")
            assert close(t, b["t"], T_TOL).all() and t[0] == 0.0, (what, i, "t", float(np.abs(t - b["t"]).max()))
            assert a.duration == t[-1] and a.v_peak == v.max() and (a.s_first, a.s_last) == (s[0], s[-1]), (what, i)
        assert (a.s_first, a.s_last) == (b["s_first"], b["s_last"]), (what, i)
        assert close(a.duration, b["duration"], T_TOL), (what, i, a.duration, b["duration"])
        if left == 0:
            assert a.v_peak == b["v_peak"] and (a.min_clearance, a.s_min_clearance) == (b["min_clearance"], b["s_min_clearance"]), (what, i)
        else:
            assert close(a.v_peak, b["v_peak"], V_TOL), (what, i)
    print("%s: %d plans, %d samples, %d undecided" % (what, len(recs), samples, undecided))
    # (one sample of a comparison of fewer than 1000 is more than the share: those count in the file's total, which the last test checks)
    assert samples < 1000 or undecided <= FR.MAX_LEFT_OUT * samples, (what, undecided, samples)
    TOTAL[0] += samples
    TOTAL[1] += undecided
    return samples, undecided


class Fleet:
    def __init__(self):
        self.s = scene()
        self.plans = restated(self.s.P)  # all N + 2
        self.grid = FR.Grid(self.s.w)


@functools.lru_cache(maxsize=None)
def fleet():
    return Fleet()


def restate(f, lim, which=None, lo=None, hi=None, vs=None, ve=None, max_samples=1 << 30, clearance=None):
    which = range(N) if which is None else which
    return [V.profile(f.plans[q], lim, -np.inf if lo is None else lo[i], np.inf if hi is None else hi[i], 0.0 if vs is None else vs[i], 0.0 if ve is None else ve[i],
                      max_samples, clearance) for i, q in enumerate(which)]


def call_kw(lim):
    return {k: v for k, v in lim.items()}


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lim", [V.limits(), V.limits(spacing=0.37, a_acc=0.8, a_dec=3.0, a_lat=0.9, dwell=1.5, v_max_forward=8.0, v_max_reverse=1.0)],
                         ids=["defaults", "spacing-0.37-dwell"])
def test_whole_plans_against_the_restatement(lim):
    """every held plan from rest to rest: a failed query (-1) among them, plans with a reverse primitive (a junction cusp), plans whose Reeds-Shepp edge
    changes direction inside; at spacing 0.37 an edge holds a fractional number of steps"""
    f = fleet()
    recs, rows = f.s.pipe.speed_profile(f.s.tickets, **call_kw(lim))
    want = restate(f, lim)
    compare(recs, rows, want, "whole plans, spacing %g" % lim["spacing"], f.s.lengths[:N])
    assert any(r.status == -1 for r in recs) and sum(r.status == 0 for r in recs) >= 40
    junction = [q for q in range(N) if f.plans[q] is not None and any(isinstance(E, R.ArcEdge) and E.backward for E in f.plans[q].edges) and recs[q].n_cusps >= 1]
    inside = [q for q in range(N) if cusp_of(f.plans[q]) is not None]
    assert junction and inside and all(recs[q].n_cusps >= 1 for q in inside)
    print("zero-length edges in the scene:", sum(int((p.L == 0.0).sum()) for p in f.plans[:N] if p is not None and p.edges))
    for q in range(N):
        if recs[q].status != 0:
            continue
        V.feasible(dict(want[q], s=rows[q][:, 0], v=rows[q][:, 1], t=rows[q][:, 2], e=rows[q][:, 1] ** 2), lim)
        assert rows[q][0, 1] == 0.0 and rows[q][-1, 1] == 0.0 and (rows[q][want[q]["cusp"], 1] == 0.0).all()
    if lim["dwell"] > 0.0:  # the dwell is the only difference to a call without one
        bare = f.s.pipe.speed_profile(f.s.tickets, samples=False, **call_kw(dict(lim, dwell=0.0)))
        for q in junction + inside:
            assert abs((recs[q].duration - bare[q].duration) - recs[q].n_cusps * lim["dwell"]) <= 1e-9 * recs[q].duration


def test_sequences_that_end_in_fill_and_pass_a_block_of_64():
    """N < 64 (one partial block), N == 64 (one full block), N == 65 (a carry into a block of one sample), N > 128 (two carries), each by a spacing
    found for some plan"""
    f = fleet()
    for what, wanted in (("N < 64", lambda n: 8 < n < 64), ("N == 64", lambda n: n == 64), ("N == 65", lambda n: n == 65), ("N == 128", lambda n: n == 128),
                         ("N == 129", lambda n: n == 129), ("N > 192", lambda n: n > 192)):
        found = V.find_spacing(f.plans[:N], wanted)
        assert found is not None, what
        q, spacing, n = found
        lim = V.limits(spacing=spacing, dwell=0.5)
        recs, rows = f.s.pipe.speed_profile(f.s.tickets[q:q + 1], v_start=1.0, v_end=0.5, **call_kw(lim))
        compare(recs, rows, restate(f, lim, [q], vs=[1.0], ve=[0.5]), "%s: plan %d at spacing %g" % (what, q, spacing), [f.s.lengths[q]])
        assert recs[0].n_samples == n and wanted(recs[0].n_samples)


def test_a_one_pose_plan_and_a_failed_query():
    """on an open 16 m box with a closed room (tests/test_gpu_pipeline_locate.py's): a goal inside the room (no plan: -1), start == goal (one pose: one
    sample at s = 0 without a direction) and a plan of a few edges beside them in one call"""
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
    # (poses off the cell borders, which lie on the multiples of 0.1: a pose on one is undecided)
    starts = np.array([(-5.0, -5.0, 0.0), (-5.03, 3.04, 0.4), (-5.03, 0.04, 0.0)])
    goals = np.array([(4.0, 4.0, 0.0), (-5.03, 3.04, 0.4), (-2.53, 0.04, 0.0)])
    pipe = pa.HybridAStarPipeline(val, capacity=4, max_nodes=32768, search_rows=4)
    pipe.initialize()
    tickets = pipe.submit(starts, goals, [50, 51, 52])
    res = drain(pipe, 3)
    assert [res[int(t)].status for t in tickets] == [-1, 0, 0] and res[int(tickets[1])].n_path == 1
    plans = restated(Plans([None] + [pipe.get_path_of(t) for t in tickets[1:]], goals, ctx))
    lengths = [r.length for r in pipe.revalidate(tickets)]
    lim = V.limits(clearance_gain=2.0, v_floor=0.1)
    clearance = V.grid_clearance(FR.Grid(w), POINT)
    for vs, ve in ((0.0, 0.0), (3.0, 1.5)):
        recs, rows = pipe.speed_profile(tickets, v_start=vs, v_end=ve, **call_kw(lim))
        compare(recs, rows, [V.profile(p, lim, v_start=vs, v_end=ve, clearance=clearance) for p in plans], "box, v_start %g" % vs, lengths)
        assert bytes(recs[0]) == bytes(C.c_int32(-1)) + bytes(68)  # every field but the status is zero
        one = recs[1]
        assert (one.status, one.n_samples, one.n_cusps, one.length, one.s_first, one.s_last, one.duration) == (0, 1, 0, 0.0, 0.0, 0.0, 0.0)
        assert rows[1].shape == (1, 3) and rows[1][0, 0] == 0.0 and rows[1][0, 2] == 0.0
        assert one.v_peak == rows[1][0, 1] == min(2.0, vs, ve)  # (without a direction the cap is v_max_reverse)
    # a window that leaves s = 0 out: no sample
    recs, rows = pipe.speed_profile(tickets, from_length=[0.0, 1e-9, 0.0], **call_kw(lim))
    compare(recs, rows, [V.profile(p, lim, lo, clearance=clearance) for p, lo in zip(plans, (0.0, 1e-9, 0.0))], "box, window")
    assert (recs[1].status, recs[1].n_samples) == (1, 0)
    pipe.close()


def test_the_clearance_term_by_footprint_point_disc_and_none():
    """gain == 0 reads no map: a target without a distance grid is accepted, and refused with gain > 0.  With a gain: the pipeline's three-disc footprint
    (CAR3), the point disc as a footprint, and no footprint (the target's min_safe_radius as a disc) -- the last two give the same bytes; min_clearance is
    the least of pp_check_states_footprint's clearances at the sample poses"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError
    f = fleet()
    s = f.s
    bare = s.fresh()
    free = s.pipe.speed_profile(s.tickets, samples=False)
    again = s.pipe.speed_profile(s.tickets, map_set=bare, samples=False)
    assert [bytes(r) for r in again] == [bytes(r) for r in free] and all(r.min_clearance == math.inf and r.s_min_clearance == 0.0 for r in free if r.status == 0)
    with pytest.raises(PPError) as e:
        s.pipe.speed_profile(s.tickets, map_set=bare, clearance_gain=1.0)
    assert e.value.code == PP_ERR_INVALID and "distance grid" in str(e.value)
    lim = V.limits(clearance_gain=1.5, v_floor=0.3)
    none = s.pipe.speed_profile(s.tickets, **call_kw(lim))
    compare(*none, restate(f, lim, clearance=V.grid_clearance(f.grid, POINT)), "no footprint", s.lengths[:N])
    lowered = sum(a.v_peak < b.v_peak for a, b in zip(none[0], free) if a.status == 0)
    assert lowered >= 10 and all(a.v_peak <= b.v_peak and a.duration >= b.duration for a, b in zip(none[0], free) if a.status == 0)
    point, car = pa.Footprint(s.ms, POINT), pa.Footprint(s.ms, FR.CAR3)
    try:
        s.pipe.set_footprint(point)
        as_disc = s.pipe.speed_profile(s.tickets, **call_kw(lim))
        assert [bytes(r) for r in as_disc[0]] == [bytes(r) for r in none[0]] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(as_disc[1], none[1]))
        s.pipe.set_footprint(car)
        recs, rows = s.pipe.speed_profile(s.tickets, **call_kw(lim))
        want = restate(f, lim, clearance=V.grid_clearance(f.grid, FR.CAR3))
        compare(recs, rows, want, "CAR3", s.lengths[:N])
        assert sum(r.min_clearance == 0.0 for r in recs if r.status == 0) >= 5  # (the plans were searched for the point: the car touches)
        for q in range(N):
            if recs[q].status != 0 or not want[q]["decided"].all():
                continue
            ok, clear = s.val.is_state_valid(want[q]["poses"], footprint=car, return_clearance=True)
            cl = np.where(ok, clear, np.float32(0)).astype(np.float64)
            assert recs[q].min_clearance == cl.min() and recs[q].s_min_clearance == want[q]["s"][int(np.argmin(cl))], q
    finally:
        s.pipe.set_footprint(None)
        point.close()
        car.close()


def test_a_wall_on_another_map_slows_the_plan_near_it_beside_a_query_in_flight():
    """map B is the scene's world plus a wall beside one plan; the pipeline searches map A with a query in flight while the profile reads B: v is lower
    near the wall and the same far from it"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    lim = V.limits(clearance_gain=1.5, v_floor=0.3)
    # the plan and the sample with the most room on map A: the wall goes 1.6 m to the left of that pose, along the plan
    on_grid = restate(f, lim, clearance=V.grid_clearance(f.grid, POINT))
    q = max((q for q in range(N) if on_grid[q]["status"] == 0), key=lambda q: float(on_grid[q]["cl"].max()))
    k = int(np.argmax(on_grid[q]["cl"]))
    assert on_grid[q]["cl"][k] > 1.0  # (more than 2 m from every obstacle: the wall becomes the nearest one)
    x, y, t = on_grid[q]["poses"][k]
    w2 = _world()
    w2.add_rectangle(0.6, 0.2, [x - 1.6 * math.sin(t), y + 1.6 * math.cos(t), t])
    w2.update()
    B = s.fresh()
    B.upload_dist2(w2.d2())
    pa.StateValidatorOccupancyMap(B)  # (the validator's tunables of B: min_safe_radius 1.0)
    flying = s.pipe.submit(s.goals[8:9], s.starts[8:9], np.array([951], dtype=np.uint64))
    assert len(flying) == 1 and s.pipe.in_flight() == 1
    on_a = s.pipe.speed_profile(s.tickets[q:q + 1], **call_kw(lim))
    on_b = s.pipe.speed_profile(s.tickets[q:q + 1], map_set=B, **call_kw(lim))
    assert s.pipe.in_flight() == 1
    drain(s.pipe, 1)
    s.pipe.release(flying)
    want_a, want_b = restate(f, lim, [q], clearance=V.grid_clearance(f.grid, POINT)), restate(f, lim, [q], clearance=V.grid_clearance(FR.Grid(w2), POINT))
    compare(*on_a, want_a, "map A", [s.lengths[q]])
    compare(*on_b, want_b, "map B", [s.lengths[q]])
    va, vb, arc = on_a[1][0][:, 1], on_b[1][0][:, 1], on_a[1][0][:, 0]
    changed = want_a[0]["cl"] != want_b[0]["cl"]
    assert changed.any() and (vb <= va).all() and (vb < va).any()
    # braking from 5 m/s takes 5 m, reaching it again 8.4 m: farther than 9 m (in arc length) from every sample whose clearance changed nothing changes
    far = np.array([np.abs(arc[changed] - u).min() > 9.0 for u in arc])
    print("%d samples, %d with another clearance, %d slower, %d far" % (len(arc), changed.sum(), (vb < va).sum(), far.sum()))
    assert np.array_equal(bits(va[far]), bits(vb[far])) and not (vb < va)[far].any()
    assert on_b[0][0].min_clearance < on_a[0][0].min_clearance or on_b[0][0].min_clearance == 0.0


def test_windows_end_speeds_and_the_sample_limit():
    """an empty window: status 1; from = the arc length of a locate result with v_start = 3: v_0 == min(cap_0, 3) unless braking for what lies ahead
    limits it; max_samples = N - 1: status -5 and untouched rows; samples_host and results_host may be NULL"""
    from pathplanning_amd._lib import SpeedProfileParams, SpeedProfileResult, ptr
    f = fleet()
    s = f.s
    lim = V.limits()
    L = np.array(s.lengths[:N])
    for what, lo, hi in (("from > length", L + 0.5, None), ("to < 0", None, np.full(N, -1e-9))):
        recs, rows = s.pipe.speed_profile(s.tickets, from_length=lo, to_length=hi)
        compare(recs, rows, restate(f, lim, lo=lo, hi=hi), what, s.lengths[:N])
        assert all((r.status, r.n_samples) == (1, 0) for r, p in zip(recs, f.plans) if p is not None)
    vehicles = np.array([p.at([1], [0.6])[0][0] if p is not None and p.edges else s.starts[q] for q, p in enumerate(f.plans[:N])])
    located = s.pipe.locate(s.tickets, vehicles, spacing=0.1)
    lo = np.array([r.s for r in located])
    hi = lo + 12.0
    vs, ve = np.full(N, 3.0), np.full(N, 2.0)
    recs, rows = s.pipe.speed_profile(s.tickets, from_length=lo, to_length=hi, v_start=vs, v_end=ve)
    want = restate(f, lim, lo=lo, hi=hi, vs=vs, ve=ve)
    compare(recs, rows, want, "from the located arc length, 12 m ahead", s.lengths[:N])
    exact = 0
    for q in range(N):
        if recs[q].status != 0:
            continue
        assert lo[q] <= recs[q].s_first <= lo[q] + 0.1 and recs[q].s_last <= hi[q]
        first = min(want[q]["cap"][0], 3.0)
        assert rows[q][0, 1] == first or (want[q]["v"][0] < first and rows[q][0, 1] < first), q
        exact += rows[q][0, 1] == first
        assert rows[q][-1, 1] <= 2.0
    assert exact >= 20
    # ---- the sample limit, through the C ABI with rows the call must not touch
    lib, pipe = s.pipe.lib, s.pipe
    q = next(q for q in range(N) if recs[q].status == 0)
    whole = pipe.speed_profile(s.tickets[q:q + 1], samples=False)[0]
    n = whole.n_samples
    t = np.ascontiguousarray(s.tickets[q:q + 1], dtype=np.uint64)
    params = SpeedProfileParams(**V.limits())
    out = (SpeedProfileResult * 1)()
    rows = np.full((1, n + 3, 3), -7.0)
    assert lib.pp_pipeline_speed_profile(pipe.h, None, 1, ptr(t), None, None, None, None, C.byref(params), n - 1, ptr(rows), out) == 0
    assert (out[0].status, out[0].n_samples, out[0].length) == (-5, n, whole.length) and all(getattr(out[0], k) == 0 for k in ZERO_FIELDS)
    assert (rows == -7.0).all()
    compare(list(out), None, restate(f, lim, [q], max_samples=n - 1), "max_samples = N - 1")
    assert lib.pp_pipeline_speed_profile(pipe.h, None, 1, ptr(t), None, None, None, None, C.byref(params), n, ptr(rows), out) == 0
    assert (out[0].status, out[0].n_samples) == (0, n) and (rows[0, :n, 0] >= 0.0).all() and (rows[0, n:] == -7.0).all()  # rows beyond n_samples stay
    assert bytes(out[0]) == bytes(whole)
    assert lib.pp_pipeline_speed_profile(pipe.h, None, 1, ptr(t), None, None, None, None, C.byref(params), n, None, out) == 0 and bytes(out[0]) == bytes(whole)
    kept = rows.copy()
    assert lib.pp_pipeline_speed_profile(pipe.h, None, 1, ptr(t), None, None, None, None, C.byref(params), n, ptr(rows), None) == 0 and np.array_equal(bits(rows), bits(kept))
    assert lib.pp_pipeline_speed_profile(pipe.h, None, 1, ptr(t), None, None, None, None, C.byref(params), n, None, None) == 0


def test_refusals_launch_nothing_and_leave_the_pipeline_usable():
    """every refusal is PP_ERR_INVALID with the first offending ticket or argument named; a valid call afterwards gives the records of before; n == 0
    is PP_OK"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError, SpeedProfileParams, SpeedProfileResult, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    first = pipe.speed_profile(held[:6], samples=False)
    out = (SpeedProfileResult * 128)()
    good = SpeedProfileParams(**V.limits())

    def refused(tickets, *words, n=None, target=None, lo=None, hi=None, vs=None, ve=None, params=good, max_samples=64):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        arrays = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi, vs, ve)]
        rc = lib.pp_pipeline_speed_profile(pipe.h, target, len(t) if n is None else n, ptr(t), *[ptr(a) for a in arrays], C.byref(params) if params is not None else None,
                                           max_samples, None, out)
        msg = lib.pp_last_error().decode()
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    refused((held + held)[:CAPACITY + 1], "capacity")
    refused(held[:1], "capacity", n=-1)
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused(held[:2], "params", params=None)
    for name in ("spacing", "v_max_forward", "v_max_reverse", "a_acc", "a_dec", "a_lat"):
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            refused(held[:2], name, "> 0", params=SpeedProfileParams(**V.limits(**{name: bad})))
    for name in ("dwell", "clearance_gain", "v_floor"):
        for bad in (-0.01, float("nan"), float("inf")):
            refused(held[:2], name, ">= 0", params=SpeedProfileParams(**V.limits(**{name: bad})))
    refused(held[:2], "max_samples", max_samples=0)
    refused(held[:2], "max_samples", max_samples=-5)
    refused(held[:3], "ticket %d" % held[2], "NaN", lo=[0.0, 1.0, float("nan")])
    refused(held[:3], "ticket %d" % held[0], "NaN", hi=[float("nan"), 1.0, 2.0])
    for bad in (float("nan"), float("inf"), -0.5):
        refused(held[:3], "ticket %d" % held[1], "v_start", vs=[0.0, bad, 1.0])
        refused(held[:3], "ticket %d" % held[2], "v_end", ve=[0.0, 1.0, bad])
    other = pa.Context(0)
    foreign = pa.OccupancyMapSet.from_bounds(other, s.w.lb, s.w.ub, 0.1)
    refused(held[:2], "another context", target=foreign.h)
    bare = s.fresh()  # (kept alive over the call)
    refused(held[:2], "distance grid", target=bare.h, params=SpeedProfileParams(**V.limits(clearance_gain=0.5)))
    # the batch form on the pipeline's buffer set
    rc = lib.pp_planner_speed_profile(pipe.planner_h, None, 1, None, None, None, None, C.byref(good), 64, None, out)
    assert rc == PP_ERR_INVALID and "pp_pipeline_speed_profile" in lib.pp_last_error().decode()
    # a query in flight: its ticket is refused; the held ones are served beside it
    flying = pipe.submit(s.goals[8:9], s.starts[8:9], np.array([950], dtype=np.uint64))
    assert len(flying) == 1 and pipe.in_flight() == 1
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "in flight")
    with pytest.raises(PPError) as e:
        pipe.speed_profile([held[0], int(flying[0])])
    assert e.value.code == PP_ERR_INVALID
    assert pipe.in_flight() == 1
    drain(pipe, 1)
    pipe.release(flying)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "released")
    with pytest.raises(ValueError):
        pipe.speed_profile(held[:3], v_start=[1.0, 2.0])
    with pytest.raises(TypeError):
        pipe.speed_profile(held[:3], jerk=1.0)
    # n == 0, and everything is as it was
    assert lib.pp_pipeline_speed_profile(pipe.h, None, 0, None, None, None, None, None, None, 64, None, out) == 0
    assert lib.pp_pipeline_speed_profile(pipe.h, None, 0, None, None, None, None, None, C.byref(good), 64, None, None) == 0
    assert pipe.speed_profile([]) == ([], [])
    again = pipe.speed_profile(held[:6], samples=False)
    assert [bytes(r) for r in again] == [bytes(r) for r in first]


def test_the_batch_form_equals_the_pipeline_form_and_the_length_is_revalidates():
    """HybridAStarBatch.speed_profile: the same kernel with identity slots on the same queries gives the same records and rows, field by field; `length`
    is revalidate's, bit for bit"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    n = 16
    batch = pa.HybridAStarBatch(s.val, max_batch=n, max_nodes=32768)
    batch.initialize(s.pipe.nonholo_table())
    res = batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
    assert sum(r.status == 0 for r in res) >= 4
    lim = V.limits(spacing=0.2, dwell=1.0, clearance_gain=1.0, v_floor=0.2)
    vs, ve = np.linspace(0.0, 3.0, n), np.linspace(2.0, 0.0, n)
    mine = batch.speed_profile(v_start=vs, v_end=ve, **call_kw(lim))
    theirs = s.pipe.speed_profile(s.tickets[:n], v_start=vs, v_end=ve, **call_kw(lim))
    for q in range(n):
        for name, _ in mine[0][q]._fields_:
            assert getattr(mine[0][q], name) == getattr(theirs[0][q], name), (q, name)
        assert np.array_equal(bits(mine[1][q]), bits(theirs[1][q])), q
    compare(*mine, restate(f, lim, range(n), vs=vs, ve=ve, clearance=V.grid_clearance(f.grid, POINT)), "batch form", [r.length for r in batch.revalidate()])
    assert [r.length for r in s.pipe.revalidate(s.tickets[:n])] == [r.length for r in theirs[0]]
    windowed = batch.speed_profile(5, from_length=1.0, to_length=3.0, spacing=0.2)
    compare(*windowed, restate(f, V.limits(spacing=0.2), range(5), lo=[1.0] * 5, hi=[3.0] * 5), "batch form, windowed")
    batch.close()


def test_the_buffers_grow_beside_a_query_in_flight():
    """more plans and more samples per plan than any call before, with a query in flight: every buffer of the service grows and the outgrown ones are
    parked, not freed (freeing waits for the grid: over a second while the host does not poll); the records and rows equal the idle call's"""
    f = fleet()
    s = f.s
    small = s.pipe.speed_profile(s.all_tickets[:2], max_samples=5000)
    flying = s.pipe.submit(s.goals[9:10], s.starts[9:10], np.array([952], dtype=np.uint64))
    assert len(flying) == 1 and s.pipe.in_flight() == 1
    t0 = time.time()
    grown = s.pipe.speed_profile(s.all_tickets, max_samples=6000)
    took = time.time() - t0
    assert s.pipe.in_flight() == 1
    print("a speed-profile call that grows its buffers beside a query in flight: %.1f ms" % (1e3 * took))
    drain(s.pipe, 1)
    s.pipe.release(flying)
    idle = s.pipe.speed_profile(s.all_tickets, max_samples=6000)
    assert [bytes(r) for r in grown[0]] == [bytes(r) for r in idle[0]] and [bytes(r) for r in grown[0][:2]] == [bytes(r) for r in small[0]]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(grown[1], idle[1]))
    assert took < 0.5


def test_the_cpp_mirror_profiles_like_a_sequential_sweep():
    """tests/cpp/test_pipeline_speed_profile.cpp: SpeedProfile(tickets) of Planner::HybridAStarPipeline against a sequential sweep over the caps"""
    from pathplanning_amd import build
    exe = build.build_pipeline_speed_profile_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"SpeedProfile(tickets) == the sweep over the plan's samples" in r.stdout


def test_the_share_of_undecided_samples_over_all_comparisons():
    """every comparison of this file so far, and one more of the whole plans: at most footprint_ref.MAX_LEFT_OUT of the samples were undecided"""
    f = fleet()
    lim = V.limits(spacing=0.05)
    compare(*f.s.pipe.speed_profile(f.s.tickets, max_samples=4096, **call_kw(lim)), restate(f, lim), "whole plans, spacing 0.05", f.s.lengths[:N])
    print("%d samples compared, %d undecided" % tuple(TOTAL))
    assert TOTAL[0] >= 20000 and TOTAL[1] <= FR.MAX_LEFT_OUT * TOTAL[0]
