"""-m gpu: vehicles located on their held plans, by ticket (pp_pipeline_locate, pp_planner_locate; k_locate_tickets in
pathplanning_amd/csrc/pp_locate.hpp; the definition is in include/pp_hip.h).

The comparator is tests/locate_restatement.py, a restatement of the two stages in numpy that shares nothing with the kernel: the plans' edges are
rebuilt from get_path_of as tests/test_gpu_pipeline_stamp.py rebuilds them (an edge's length is the plan's own bits; arc poses from the closed form of
ConstantSteer in numpy, Reeds-Shepp poses from pp_rs_path_interpolate on records built from the plan's word and t, u, v).

On every case status, n_samples and length are EQUAL (length to revalidate's).  A case is DECIDED when the restatement's best candidate beats, by more
than EPS = 1e-9 m^2, every other stage-2 candidate and every stage-1 sample farther than 2 * spacing from it (device and glibc poses differ around
1e-12 m; a lever of 40 m gives 1e-10 m^2).  On a decided case edge, direction and s are EQUAL and ratio, pose, distance, along, lateral and
heading_error agree within 1e-9.  On an undecided case the cost of the device's (edge, ratio), evaluated by the restatement, is within EPS of the
restatement's minimum.  At most 2 % of the cases of a comparison may be undecided (expected: about 1e-4 per case);
tests/test_locate_restatement_host.py checks on the CPU, with the oracle's plans of the same queries, that the restatement alone stays within that.

Scene: the one of tests/test_gpu_pipeline_stamp.py (synthetic_world(256, 14, 3), validator (1.0, 0.1), 48 plans held in a capacity-64 pipeline, shared
with that file when both run in one process).  Vehicles per plan, RandomState(SEED): five points of the plan at arbitrary s pushed sideways by up to
0.5 m and turned by up to 0.3 rad, the exact start pose, the exact goal pose, one pose 40 m outside the map.  Every test leaves the pipeline without
a footprint and with nothing in flight."""
import ctypes as C
import functools
import math
import os
import subprocess
import time

import numpy as np
import pytest

import locate_restatement as R
import oracle_lib as O
from test_gpu_pipeline_stamp import CAPACITY, N, RES, Geometry, Plans, drain, expect, scene
from test_gpu_pipeline_stamp import compare as compare_stamp
from test_locate_restatement_host import SEED, cusp_of

pytestmark = pytest.mark.gpu

EPS = R.EPS
TOL = 1e-9
MAX_UNDECIDED = 0.02
PP_ERR_INVALID = -1
HALF = 128 * RES
FIELDS = ("edge", "direction", "s", "ratio", "distance", "along", "lateral", "heading_error")


def restated(P):
    """the plans of a test_gpu_pipeline_stamp.Plans object as the restatement's edge objects"""
    out = []
    for q, p in enumerate(P.plans):
        if p is None or len(p["poses"]) == 0:
            out.append(None)
            continue
        edges = []
        for e in range(1, len(p["poses"])):
            L, prim = float(p["length"][e]), int(p["prim"][e])
            edges.append(R.ArcEdge(p["poses"][e - 1], L, P.curv[prim], P.direc[prim]) if p["kind"][e] == 1 else R.RsEdge(P.rs[q], L, P.rsp.interpolate))
        out.append(R.Plan(p["poses"][0], edges))
    return out


def compare(got, want, what, lengths=None):
    """the records of the device against the restatement's, case by case; returns the number of undecided cases"""
    assert len(got) == len(want)
    undecided = 0
    for i, (a, b) in enumerate(zip(got, want)):
        print("%s case %3d: status %d samples %d edge %d dir %d s %.17g ratio %.17g dist %.17g lat %.17g dth %.17g length %.17g | want status %d samples %d edge %d s %.17g %s" %
              (what, i, a.status, a.n_samples, a.edge, a.direction, a.s, a.ratio, a.distance, a.lateral, a.heading_error, a.length, b["status"], b["n_samples"], b["edge"], b["s"],
               "" if b["status"] != 0 or b["decided"] else "UNDECIDED"))
        assert (a.status, a.n_samples) == (b["status"], b["n_samples"]) and a.length == b["length"], (what, i)
        if lengths is not None:
            assert a.length == lengths[i], (what, i)
        if b["status"] != 0:
            assert all(getattr(a, f) == 0 for f in FIELDS) and tuple(a.pose) == (0.0, 0.0, 0.0), (what, i)
            continue
        if not b["decided"]:
            undecided += 1
            c = b["cost_at"](a.edge, a.ratio)
            print("    the device's (edge, ratio) costs %.17g, the restatement's minimum is %.17g" % (c, b["c"]))
            assert abs(c - b["c"]) <= EPS, (what, i, c, b["c"])
            continue
        assert (a.edge, a.direction) == (b["edge"], b["direction"]) and a.s == b["s"], (what, i, a.edge, b["edge"], a.s, b["s"])
        for f in FIELDS[3:]:
            assert abs(getattr(a, f) - b[f]) <= TOL, (what, i, f, getattr(a, f), b[f])
        assert max(abs(x - y) for x, y in zip(a.pose, b["pose"])) <= TOL, (what, i, tuple(a.pose), b["pose"])
    print("%s: %d cases, %d undecided" % (what, len(got), undecided))
    assert undecided <= MAX_UNDECIDED * len(got), (what, undecided, len(got))
    return undecided


class Fleet:
    def __init__(self):
        self.s = scene()
        self.plans = restated(self.s.P)
        rng = np.random.RandomState(SEED)
        self.vehicles = np.array([R.vehicle_poses(self.plans[q], self.s.starts[q], self.s.goals[q], HALF, rng) for q in range(N)])  # [N, 8, 3]
        self.kinds = self.vehicles.shape[1]


@functools.lru_cache(maxsize=None)
def fleet():
    return Fleet()


def locate_all(f, spacing, w, lo=None, hi=None):
    """one call per kind of vehicle pose over the 48 tickets; (records, restatement) over all N * kinds cases, plan-major within a kind"""
    got, want = [], []
    for k in range(f.kinds):
        got += f.s.pipe.locate(f.s.tickets, f.vehicles[:, k], from_length=lo, to_length=hi, spacing=spacing, heading_weight=w)
        want += [R.locate(f.plans[q], f.vehicles[q, k], spacing, w, -np.inf if lo is None else lo[q], np.inf if hi is None else hi[q]) for q in range(N)]
    return got, want


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,weight", [(0.1, 0.0), (0.37, 0.0), (0.1, 2.0)])
def test_vehicles_beside_on_and_far_from_their_plans(spacing, weight):
    """spacings 0.1 and 0.37 (an edge holds a fractional number of steps), and 0.1 with a heading weight; the exact start pose is found at s = 0, the
    exact goal pose at the plan's end, a pose 40 m outside the map at 39 m and more"""
    f = fleet()
    got, want = locate_all(f, spacing, weight)
    compare(got, want, "spacing %g, weight %g" % (spacing, weight), f.s.lengths[:N] * f.kinds)
    solved = [q for q in range(N) if f.plans[q] is not None and f.plans[q].edges]
    assert len(solved) >= 40
    for q in solved:
        near, start, goal, far = got[q:5 * N:N], got[5 * N + q], got[6 * N + q], got[7 * N + q]
        assert all(r.status == 0 and r.distance <= math.hypot(0.5, weight * 0.3) + spacing / 32 for r in near), q
        assert (start.edge, start.s, start.ratio, start.distance) == (1, 0.0, 0.0, 0.0) and tuple(start.pose) == tuple(f.s.starts[q])
        assert goal.edge == len(f.plans[q].edges) and goal.length - goal.s <= spacing / 32 and goal.distance < 1e-6
        assert far.distance >= R.OUTSIDE - 1.0 and far.status == 0
    if spacing == 0.37:
        assert any(R.steps(p.L[0], spacing) * spacing != p.L[0] for p in f.plans[:N] if p is not None and p.edges)


def test_spacing_of_a_centimetre_on_one_plan():
    """an edge of more than 64 samples (several passes of the wave over one edge) and a lattice step of 0.3 mm"""
    f = fleet()
    q = max((q for q in range(N) if f.plans[q] is not None and f.plans[q].edges), key=lambda q: f.plans[q].L.max())
    assert R.steps(f.plans[q].L.max(), 0.01) > 64
    got = [f.s.pipe.locate(f.s.tickets[q:q + 1], v[None], spacing=0.01)[0] for v in f.vehicles[q]]
    want = [R.locate(f.plans[q], v, 0.01) for v in f.vehicles[q]]
    compare(got, want, "spacing 0.01, plan %d" % q, [f.s.lengths[q]] * f.kinds)
    assert all(r.n_samples > 64 for r in got)
    # the resolution is what was asked for: a point of the plan is found within half a lattice step along it
    for u in (0.3, 0.61803):
        e = int(np.searchsorted(f.plans[q].S, u * f.plans[q].length, side="right"))
        pose = f.plans[q].at([e], [0.37])[0][0]
        r = f.s.pipe.locate(f.s.tickets[q:q + 1], pose[None], spacing=0.01)[0]
        assert r.edge == e and r.distance <= 0.5 * 0.01 / 32 + 1e-9 and abs(r.ratio - 0.37) * f.plans[q].L[e - 1] <= 0.5 * 0.01 / 32 + 1e-9


def test_a_plan_of_more_than_64_edges():
    """corner to corner on the 1024^2 world (87 poses in the oracle: lanes take a second edge in the prologue, and the binary searches run over more
    than 64 entries)"""
    import pathplanning_amd as pa
    from gpu_common import make_pair
    w, ms, val, ctx = make_pair(1024, 24, 1)
    pipe = pa.HybridAStarPipeline(val, capacity=4, max_nodes=65536, search_rows=4)
    pipe.initialize()
    starts, goals = np.array([[-48.0, -48.0, 0.0]]), np.array([[48.0, 48.0, 0.0]])
    tickets = pipe.submit(starts, goals, [7])
    res = drain(pipe, 1)
    assert res[int(tickets[0])].status == 0 and res[int(tickets[0])].n_path > 65
    plan, = restated(Plans([pipe.get_path_of(tickets[0])], goals, ctx))
    length = pipe.revalidate(tickets)[0].length
    vehicles = R.vehicle_poses(plan, starts[0], goals[0], 51.2, np.random.RandomState(SEED), n_random=13)
    for spacing, w8 in ((0.1, 0.0), (0.37, 1.0)):
        got = [pipe.locate(tickets, v[None], spacing=spacing, heading_weight=w8)[0] for v in vehicles]
        compare(got, [R.locate(plan, v, spacing, w8) for v in vehicles], "87-pose plan, spacing %g" % spacing, [length] * len(vehicles))
        assert max(r.edge for r in got) > 64 and min(r.edge for r in got) == 1
    pipe.close()


def test_a_one_pose_plan_and_a_failed_query():
    """on an open 16 m box with a closed room (tests/test_gpu_pipeline_revalidate.py's): a goal inside the room (no plan: -1), start == goal (one pose,
    one sample at s = 0, edge 0, no second stage), and a plan of a few edges beside them in one call"""
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
    starts = np.array([(-5.0, -5.0, 0.0), (-5.0, 3.0, 0.4), (-5.0, 0.0, 0.0)])
    goals = np.array([(4.0, 4.0, 0.0), (-5.0, 3.0, 0.4), (-2.5, 0.0, 0.0)])
    pipe = pa.HybridAStarPipeline(val, capacity=4, max_nodes=32768, search_rows=4)
    pipe.initialize()
    tickets = pipe.submit(starts, goals, [50, 51, 52])
    res = drain(pipe, 3)
    assert [res[int(t)].status for t in tickets] == [-1, 0, 0] and res[int(tickets[1])].n_path == 1
    plans = restated(Plans([None] + [pipe.get_path_of(t) for t in tickets[1:]], goals, ctx))
    lengths = [r.length for r in pipe.revalidate(tickets)]
    vehicles = np.array([(-4.0, -4.0, 1.0), (-4.7, 3.4, -2.0), (-4.0, 0.3, 0.2)])
    got = pipe.locate(tickets, vehicles, spacing=0.1, heading_weight=0.5)
    compare(got, [R.locate(plans[i], vehicles[i], 0.1, 0.5) for i in range(3)], "box", lengths)
    assert bytes(got[0]) == bytes(C.c_int32(-1)) + bytes(92)  # every field but the status is zero
    one = got[1]
    assert (one.status, one.edge, one.direction, one.n_samples, one.s, one.ratio, one.length) == (0, 0, 1, 1, 0.0, 0.0, 0.0)
    assert tuple(one.pose) == (-5.0, 3.0, 0.4) and abs(one.distance - 0.5) < 1e-12 and abs(one.heading_error - (-2.4)) < 1e-12
    # a window that leaves s = 0 out: no sample
    out = pipe.locate(tickets, vehicles, from_length=[0.0, 1e-9, 0.0], spacing=0.1)
    compare(out, [R.locate(plans[i], vehicles[i], 0.1, 0.0, lo) for i, lo in enumerate((0.0, 1e-9, 0.0))], "box, window")
    assert (out[1].status, out[1].n_samples) == (1, 0)
    pipe.close()


def test_a_cusp_the_heading_weight_and_a_window_choose_the_branch():
    """a plan that ends in a Reeds-Shepp edge with a cusp: a vehicle half-way between the points `a` metres before and behind the cusp is equally near
    both branches in position.  With heading_weight 0 its heading does not matter; with 2.0 it is found on the branch whose heading it has; a window
    that starts at the cusp selects the other branch all the same."""
    f = fleet()
    found = [(q, cusp_of(f.plans[q])) for q in range(N) if cusp_of(f.plans[q]) is not None]
    found = [(q, c) for q, c in found if min(c[1], 1.0 - c[1]) * f.plans[q].L[-1] > 0.8]
    assert found, "no plan with a cusp 0.8 m inside its Reeds-Shepp edge"
    checked = 0
    for q, (sc, rc) in found[:4]:
        plan, ticket = f.plans[q], f.s.tickets[q:q + 1]
        L, e = plan.L[-1], len(plan.edges)
        a = 0.75
        (before, behind), _ = plan.at([e, e], [rc - a / L, rc + a / L])
        apart = abs((before[2] - behind[2]) - R.TWO_PI * round((before[2] - behind[2]) / R.TWO_PI))
        if apart < 0.3:
            continue  # (a straight motion on one side: the branches share their heading)
        mid = 0.5 * (before[:2] + behind[:2])
        cases = []
        for heading, w, lo in ((before[2], 0.0, None), (behind[2], 0.0, None), (before[2], 2.0, None), (behind[2], 2.0, None), (before[2], 2.0, sc)):
            v = np.array([mid[0], mid[1], heading])
            got = f.s.pipe.locate(ticket, v[None], from_length=None if lo is None else [lo], spacing=0.1, heading_weight=w)[0]
            cases.append((got, R.locate(plan, v, 0.1, w, -np.inf if lo is None else lo)))
        compare([g for g, _ in cases], [b for _, b in cases], "cusp of plan %d at s = %.3f" % (q, sc), [f.s.lengths[q]] * 5)
        free_a, free_b, on_a, on_b, windowed = (g for g, _ in cases)
        assert free_a.s == free_b.s and free_a.distance == free_b.distance  # without a weight the heading chooses nothing
        assert on_a.s < sc < on_b.s and abs(on_a.heading_error) < 0.15 and abs(on_b.heading_error) < 0.15
        assert windowed.status == 0 and windowed.s >= sc
        checked += 1
    assert checked >= 1


def test_windows_empty_and_cutting_the_lattice():
    """from > length and to < 0: status 1 with n_samples 0, every other field zero but the length; a window of 12.6 cm that starts 1.3 cm before the
    point found without a window, so that it cuts the lattice range on both sides"""
    f = fleet()
    L = np.array(f.s.lengths[:N])
    for what, lo, hi in (("from > length", L + 0.5, None), ("to < 0", None, np.full(N, -1e-9))):
        got = f.s.pipe.locate(f.s.tickets, f.vehicles[:, 0], from_length=lo, to_length=hi, spacing=0.1)
        want = [R.locate(f.plans[q], f.vehicles[q, 0], 0.1, 0.0, -np.inf if lo is None else lo[q], np.inf if hi is None else hi[q]) for q in range(N)]
        compare(got, want, what, f.s.lengths[:N])
        assert all((r.status, r.n_samples) == (1, 0) for r, p in zip(got, f.plans) if p is not None)
    free = f.s.pipe.locate(f.s.tickets, f.vehicles[:, 1], spacing=0.1)
    lo = np.array([r.s for r in free]) - 0.013
    hi = lo + 0.126
    got, want = locate_all(f, 0.1, 0.0, lo, hi)
    compare(got, want, "a window that cuts the lattice", f.s.lengths[:N] * f.kinds)
    located = [(r, q % N) for q, r in enumerate(got) if r.status == 0]
    assert len(located) >= 250 and all(lo[q] <= r.s <= hi[q] for r, q in located)
    assert all(1 <= r.n_samples <= 4 for r, q in located)  # (one or two sample positions, a junction's counted twice)


def test_beside_queries_in_flight():
    """eight queries submitted on the pipeline's map and not polled; the call runs beside them and matches the restatement; the queries then complete
    with the batch planner's results"""
    import pathplanning_amd as pa
    f = fleet()
    s = f.s
    fs, fg, fz = np.ascontiguousarray(s.goals[:8]), np.ascontiguousarray(s.starts[:8]), np.arange(8, dtype=np.uint64) + 900
    batch = pa.HybridAStarBatch(s.val, max_batch=8, max_nodes=32768)
    batch.initialize(s.pipe.nonholo_table())
    ref = batch.search_batch(fs, fg, fz)
    flying = s.pipe.submit(fs, fg, fz)
    assert len(flying) == 8 and s.pipe.in_flight() == 8
    t0 = time.time()
    got = s.pipe.locate(s.tickets, f.vehicles[:, 2], spacing=0.1, heading_weight=1.0)
    print("locate of %d held plans beside 8 queries in flight: %.2f ms" % (N, 1e3 * (time.time() - t0)))
    assert s.pipe.in_flight() == 8  # nothing was polled
    compare(got, [R.locate(f.plans[q], f.vehicles[q, 2], 0.1, 1.0) for q in range(N)], "beside queries in flight", s.lengths[:N])
    fresh = drain(s.pipe, 8)
    for i, t in enumerate(flying):
        r = fresh[int(t)]
        assert (r.status, r.n_expanded, r.n_path, r.cost) == (ref[i].status, ref[i].n_expanded, ref[i].n_path, ref[i].cost)
    s.pipe.release(flying)
    batch.close()


def test_refusals_launch_nothing_and_leave_the_pipeline_usable():
    """every refusal is PP_ERR_INVALID with the first offending ticket or argument named; a valid call afterwards gives the records of before; n == 0
    is PP_OK"""
    from pathplanning_amd._lib import LocateParams, LocateResult, PPError, ptr
    f = fleet()
    s = f.s
    lib, pipe = s.pipe.lib, s.pipe
    held = [int(t) for t in s.tickets]
    poses = np.ascontiguousarray(f.vehicles[:, 3])
    first = pipe.locate(held[:6], poses[:6], spacing=0.1, heading_weight=0.5)
    out = (LocateResult * 128)()
    good = LocateParams(0.1, 0.5)

    def refused(tickets, *words, n=None, v=poses, lo=None, hi=None, params=good):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        v = None if v is None else np.ascontiguousarray(np.resize(v, (max(len(t), 1), 3)) if len(v) < len(t) else v, dtype=np.float64)
        a = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
        b = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
        rc = lib.pp_pipeline_locate(pipe.h, len(t) if n is None else n, ptr(t), ptr(v), ptr(a), ptr(b), C.byref(params) if params is not None else None, out)
        msg = lib.pp_last_error().decode()
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    refused((held + held)[:CAPACITY + 1], "capacity")
    refused(held[:1], "capacity", n=-1)
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused(held[:2], "params", params=None)
    refused(held[:2], "poses_host", v=None)
    for spacing in (0.0, -0.1, float("nan"), float("inf")):
        refused(held[:2], "spacing", params=LocateParams(spacing, 0.0))
    for weight in (-0.01, float("nan"), float("inf")):
        refused(held[:2], "heading_weight", params=LocateParams(0.1, weight))
    for k, bad in enumerate((float("nan"), float("inf"), -float("inf"))):
        v = poses[:3].copy()
        v[2 - k, k] = bad
        refused(held[:3], "ticket %d" % held[2 - k], "not finite", v=v)
    refused(held[:3], "ticket %d" % held[2], "NaN", lo=[0.0, 1.0, float("nan")])
    refused(held[:3], "ticket %d" % held[0], "NaN", hi=[float("nan"), 1.0, 2.0])
    # a query in flight: its ticket is refused; the held ones are served beside it
    flying = pipe.submit(s.goals[8:9], s.starts[8:9], np.array([950], dtype=np.uint64))
    assert len(flying) == 1 and pipe.in_flight() == 1
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "in flight")
    with pytest.raises(PPError) as e:
        pipe.locate([held[0], int(flying[0])], poses[:2])
    assert e.value.code == PP_ERR_INVALID
    assert pipe.in_flight() == 1
    drain(pipe, 1)
    pipe.release(flying)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "released")
    with pytest.raises(ValueError):
        pipe.locate(held[:3], poses[:2])
    # n == 0, and everything is as it was
    assert lib.pp_pipeline_locate(pipe.h, 0, None, None, None, None, None, out) == 0
    assert lib.pp_pipeline_locate(pipe.h, 0, None, None, None, None, C.byref(good), None) == 0
    assert pipe.locate([], np.empty((0, 3))) == []
    again = pipe.locate(held[:6], poses[:6], spacing=0.1, heading_weight=0.5)
    assert [bytes(r) for r in again] == [bytes(r) for r in first]
    assert lib.pp_pipeline_locate(pipe.h, 6, ptr(np.ascontiguousarray(held[:6], dtype=np.uint64)), ptr(poses), None, None, C.byref(good), None) == 0  # (the records are optional)


def test_a_ticket_released_by_any_route_is_refused_afterwards():
    """pp_pipeline_release, pp_pipeline_get_paths with release, pp_pipeline_get_processed_paths with release, pp_pipeline_poll with release: the ticket
    is refused by name afterwards, and the tickets still held are located as before"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError
    from gpu_common import make_pair
    from test_gpu_pipeline_release_routes import SPACING, poll_all, short_queries
    w, ms, val, ctx = make_pair(96, 3, 5)
    ms.upload_nearest_cells(*O.world_nearest(w))
    starts, goals = short_queries(w, 7)
    seeds = np.arange(7, dtype=np.uint64) + 50
    pipe = pa.HybridAStarPipeline(val, capacity=8, max_nodes=32768, search_rows=4)
    pipe.initialize()
    held = [int(t) for t in pipe.submit(starts[:6], goals[:6], seeds[:6])]
    poll_all(pipe, 6, release=False)
    vehicle = {t: starts[i] + (0.1, -0.2, 0.05) for i, t in enumerate(held)}
    before = {t: bytes(pipe.locate([t], vehicle[t][None], spacing=0.1)[0]) for t in held}

    def check_released(t):
        with pytest.raises(PPError) as e:
            pipe.locate(held + [t], np.array([vehicle[x] for x in held + [t]]))
        assert e.value.code == PP_ERR_INVALID and "ticket %d" % t in str(e.value) and "released" in str(e.value), str(e.value)
        now = pipe.locate(held, np.array([vehicle[x] for x in held]), spacing=0.1)
        assert [bytes(r) for r in now] == [before[x] for x in held], t

    t = held.pop(2)
    pipe.release([t])
    check_released(t)
    t = held.pop(0)
    pipe.get_paths([t], max_poses=64, release=True)
    check_released(t)
    t = held.pop(1)
    pipe.postprocess(held + [t], path_interpolation=SPACING)
    pipe.get_processed_paths([t], release=True)
    check_released(t)
    seventh = [int(x) for x in pipe.submit(starts[6:], goals[6:], seeds[6:])]
    vehicle[seventh[0]] = starts[6]
    assert sorted(poll_all(pipe, 1, release=True)) == seventh
    check_released(seventh[0])
    assert len(held) == 3 and pipe.in_flight() == 0
    pipe.close()


def test_the_batch_form_on_a_one_wave_planner():
    """HybridAStarBatch.locate: the same kernel with identity slots, against the same restatement; a planner that is a pipeline's buffer set is
    refused"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import LocateParams, LocateResult, ptr
    f = fleet()
    s = f.s
    n = 16
    batch = pa.HybridAStarBatch(s.val, max_batch=n, max_nodes=32768)
    assert batch.search_rows == 0
    batch.initialize(s.pipe.nonholo_table())
    res = batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
    plans = [batch.get_path_of(q) if res[q].status == 0 else None for q in range(n)]
    assert sum(p is not None for p in plans) >= 4
    mine = restated(Plans(plans, s.goals[:n], s.ctx))
    lengths = [r.length for r in batch.revalidate()]
    for k in (0, 4, 7):
        got = batch.locate(f.vehicles[:n, k], spacing=0.2, heading_weight=0.3)
        compare(got, [R.locate(mine[q], f.vehicles[q, k], 0.2, 0.3) for q in range(n)], "batch form, vehicles %d" % k, lengths)
    got = batch.locate(f.vehicles[:5, 1], 5, from_length=1.0, to_length=3.0, spacing=0.2)
    compare(got, [R.locate(mine[q], f.vehicles[q, 1], 0.2, 0.0, 1.0, 3.0) for q in range(5)], "batch form, windowed", lengths[:5])
    out = (LocateResult * 4)()
    v = np.zeros((1, 3))
    rc = s.pipe.lib.pp_planner_locate(s.pipe.planner_h, 1, ptr(v), None, None, C.byref(LocateParams(0.1, 0.0)), out)
    assert rc == PP_ERR_INVALID and "pp_pipeline_locate" in s.pipe.lib.pp_last_error().decode()
    rc = s.pipe.lib.pp_planner_locate(batch.h, n + 1, ptr(np.zeros((n + 1, 3))), None, None, C.byref(LocateParams(0.1, 0.0)), out)
    assert rc == PP_ERR_INVALID
    batch.close()


def test_the_cpp_mirror_locates_like_its_path_objects():
    """tests/cpp/test_pipeline_locate.cpp: Locate(tickets, poses) of Planner::HybridAStarPipeline against HybridAStar::GetGraphSearchPath's path objects
    searched candidate by candidate"""
    from pathplanning_amd import build
    exe = build.build_pipeline_locate_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"Locate(tickets, poses) == the least cost over the path objects' candidates" in r.stdout


def test_a_stamp_from_the_located_arc_length_reserves_what_lies_ahead():
    """the loop the call exists for: stamp with from_length = the located s reserves exactly the samples with s >= that value -- their number, and the
    cells the stamp's own restatement gives for that window"""
    f = fleet()
    s = f.s
    got = s.pipe.locate(s.tickets, f.vehicles[:, 4], spacing=0.1)
    compare(got, [R.locate(f.plans[q], f.vehicles[q, 4], 0.1) for q in range(N)], "before the stamp", s.lengths[:N])
    driven = np.array([r.s for r in got])
    B = s.fresh()
    stamped = s.pipe.stamp(s.tickets, map_set=B, from_length=driven, spacing=0.1, values=4)
    ahead = 0
    for q in range(N):
        if f.plans[q] is None:
            assert (stamped[q].status, stamped[q].n_samples) == (-1, 0)
            continue
        arc = f.plans[q].samples(0.1)[2] if f.plans[q].edges else np.zeros(1)
        assert stamped[q].n_samples == int((arc >= driven[q]).sum()), q
        assert stamped[q].n_samples < len(arc) or driven[q] == 0.0
        ahead += stamped[q].n_samples
    assert ahead > 1000
    compare_stamp(stamped, B.download_occupancy(), expect(s.P, list(range(N)), Geometry(B), s.point, 0.0, 0.1, values=[4] * N, lo=driven), "ahead of the vehicles", s.lengths[:N])
