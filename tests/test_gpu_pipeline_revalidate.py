"""-m gpu: held plans re-checked against a changed map, by ticket (pp_pipeline_revalidate, pp_planner_revalidate; k_revalidate_tickets in
pathplanning_amd/csrc/pp_revalidate.hpp).  The expected verdicts come from code the new kernel shares nothing with at run time: every
plan's edges are rebuilt on the host from get_path_of (arc curvature from the primitive index, the Reeds-Shepp edge through
ReedsSheppPaths.connect) and marched by the validator's existing entry points (pp_check_arcs[_footprint], pp_check_rs_paths[_footprint],
pp_check_states[_footprint]): status, blocked edge, ratio and both lengths must be EQUAL.  The same edge data goes through the CPU oracle
(World.is_path_valid_csteer, rs_paths_valid: equal, as in test_gpu_parity.py / test_gpu_paths.py) and, with a footprint, through
tests/footprint_ref.py outside its guard band.

The scenario was fixed with the oracle on the CPU: world make_pair(256, 6, 3), 48 valid random queries of RandomState(77), seeds 1200 ..;
48 are solved (2 to 18 poses), none blocked on the map as it was; with a 12 m x 0.5 m wall at (0, 0, 0.3) 23 are blocked (13 on an arc, 10
on the final Reeds-Shepp edge, first blocked edges 1 to 10) and 25 stay valid."""
import os
import subprocess
import time

import numpy as np
import pytest

import footprint_ref as R
import oracle_lib as O
from gpu_common import make_pair, valid_random_poses

pytestmark = pytest.mark.gpu

N, CAPACITY = 48, 64
WALL = (12.0, 0.5, (0.0, 0.0, 0.3))
PP_ERR_INVALID = -1  # include/pp_hip.h
FIELDS = ("status", "n_edges", "blocked_edge", "blocked_ratio", "valid_length", "length")


def drain(pipe, want, timeout=120.0):
    """polls with hold until `want` results have arrived; returns {ticket: QueryResult}"""
    got = {}
    t0 = time.time()
    while len(got) < want:
        tickets, res = pipe.poll(4096, release=False)
        for i, t in enumerate(tickets):
            got[int(t)] = res[i]
        if not len(tickets):
            time.sleep(0.001)
        assert time.time() - t0 < timeout, "pipeline stalled: %d of %d results" % (len(got), want)
    return got


def as_tuples(results):
    return [tuple(getattr(r, f) for f in FIELDS) for r in results]


class Edges:
    """the edges of a list of plans (get_path_of dicts; None = no plan) as flat arrays for the check entry points: arcs (start pose,
    primitive, length), Reeds-Shepp edges (records of ReedsSheppPaths.connect(parent pose, goal), whose word must be the logged one),
    and every plan's last pose"""

    def __init__(self, plans, goals, ctx):
        import pathplanning_amd as pa
        self.plans = plans
        self.steer, self.curv, self.direc = pa.HybridAStarSearchParameters().primitives()
        arc_from, self.arc_prim, arc_len, self.arc_at, rs_from, rs_goal, rs_word, self.rs_at, last, self.last_at = [], [], [], [], [], [], [], [], [], []
        self.rs_len = []
        for q, p in enumerate(plans):
            if p is None or len(p["poses"]) == 0:
                continue
            last.append(p["poses"][-1])
            self.last_at.append(q)
            for e in range(1, len(p["poses"])):
                if p["kind"][e] == 1:
                    arc_from.append(p["poses"][e - 1])
                    self.arc_prim.append(int(p["prim"][e]))
                    arc_len.append(p["length"][e])
                    self.arc_at.append((q, e))
                else:
                    assert p["kind"][e] == 2 and e == len(p["poses"]) - 1  # the analytic expansion ends the plan
                    rs_from.append(p["poses"][e - 1])
                    rs_goal.append(goals[q])
                    rs_word.append(int(p["prim"][e]))
                    self.rs_len.append(float(p["length"][e]))
                    self.rs_at.append((q, e))
        self.arc_from, self.arc_len = np.array(arc_from).reshape(-1, 3), np.array(arc_len)
        self.arc_prim = np.array(self.arc_prim, dtype=np.int64)
        self.last = np.array(last).reshape(-1, 3)
        self.rs = np.zeros(0, dtype=O.RS_PATH_DTYPE)
        if rs_from:
            self.rs = pa.ReedsSheppPaths(ctx, min_turning_radius=2.0).connect(np.array(rs_from).reshape(-1, 3), np.array(rs_goal).reshape(-1, 3))
        assert np.array_equal(self.rs["word"], np.array(rs_word, dtype=np.int32))
        # An edge's LENGTH is the plan's own, as get_path_of hands it out for arcs and for the Reeds-Shepp edge alike (the search stored
        # PathSegment::GetLength of the word it logged).  connect() solves the word again from the parent's freshly computed sin / cos, the
        # search solved it from the sin / cos stored with the node, so its t, u, v -- and its record's length -- may differ from the plan's
        # in the last bits (seen: 2 ulp on a 14 m plan); they agree to 1e-9.
        if rs_from:
            assert np.abs(self.rs["length"] - np.array(self.rs_len)).max() < 1e-9
        self.n_edges = len(self.arc_at) + len(self.rs_at)

    def verdicts(self, arc_valid, arc_last, rs_valid, rs_last, last_valid):
        """(status, n_edges, blocked_edge, blocked_ratio, valid_length, length) per plan from per-edge verdicts; lengths summed root first"""
        ok, ratio, length = {}, {}, {}
        for i, at in enumerate(self.arc_at):
            ok[at], ratio[at], length[at] = bool(arc_valid[i]), np.float32(arc_last[i]), float(self.arc_len[i])
        for i, at in enumerate(self.rs_at):
            ok[at], ratio[at], length[at] = bool(rs_valid[i]), np.float32(rs_last[i]), self.rs_len[i]
        goal_ok = {q: bool(last_valid[i]) for i, q in enumerate(self.last_at)}
        out = []
        for q, p in enumerate(self.plans):
            if p is None or len(p["poses"]) == 0:
                out.append((-1, 0, 0, np.float32(1.0), 0.0, 0.0))
                continue
            n = len(p["poses"]) - 1
            total, blocked, valid_length = 0.0, 0, None
            for e in range(1, n + 1):
                if blocked == 0 and not ok[(q, e)]:
                    blocked = e
                    valid_length = total + float(ratio[(q, e)]) * length[(q, e)]
                total = total + length[(q, e)]
            if blocked:
                out.append((1, n, blocked, ratio[(q, blocked)], valid_length, total))
            else:
                out.append((0 if goal_ok[q] else 2, n, 0, np.float32(1.0), total, total))
        return out

    def by_validator(self, val, footprint=None):
        """the existing entry points of the library on val's map as it is now"""
        av, al = val.is_path_valid(self.arc_from, self.curv[self.arc_prim], self.arc_len, self.direc[self.arc_prim], footprint=footprint) if len(self.arc_at) else ([], [])
        rv, rl = val.is_rs_path_valid(self.rs, footprint=footprint) if len(self.rs_at) else ([], [])
        lv = val.is_state_valid(self.last, footprint=footprint) if len(self.last_at) else []
        return self.verdicts(av, al, rv, rl, lv)

    def by_oracle(self, w):
        """the CPU oracle on the world as it is now (point validator)"""
        av, al = w.is_path_valid_csteer(self.arc_from, self.steer[self.arc_prim], self.arc_len, self.direc[self.arc_prim]) if len(self.arc_at) else ([], [])
        rv, rl = O.rs_paths_valid(w, self.rs) if len(self.rs_at) else ([], [])
        lv = w.is_state_valid(self.last) if len(self.last_at) else []
        return self.verdicts(av, al, rv, rl, lv)

    def by_footprint_ref(self, g, discs):
        """tests/footprint_ref.py on Grid g; also the plans with an edge or a last pose in its guard band"""
        av, al, ag, _ = R.fp_arcs(g, self.arc_from, self.curv[self.arc_prim], self.arc_len, self.direc[self.arc_prim], discs)
        rv, rl, rg, _ = R.fp_rs_paths(g, self.rs, discs)
        lv, _, _, lg = R.fp_state(g, self.last, discs)
        guarded = {q for i, (q, e) in enumerate(self.arc_at) if ag[i]} | {q for i, (q, e) in enumerate(self.rs_at) if rg[i]} | {q for i, q in enumerate(self.last_at) if lg[i]}
        return self.verdicts(av, al, rv, rl, lv), guarded


def same_exactly(got, want, what):
    """revalidate's records against a comparator's tuples: every field equal"""
    assert len(got) == len(want)
    for q, (a, b) in enumerate(zip(as_tuples(got), want)):
        print("%s plan %2d: got %s want %s" % (what, q, a, tuple(b)))
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], (what, q, a, b)
        assert np.float32(a[3]) == np.float32(b[3]) and a[4] == b[4] and a[5] == b[5], (what, q, a, b)


def same_verdict_and_ratio(got, want, what, skip=()):
    """against the oracle / the numpy restatement: status and blocked edge equal, the ratio equal as test_gpu_parity.py / test_gpu_paths.py
    compare `last` (np.array_equal)"""
    for q, (a, b) in enumerate(zip(as_tuples(got), want)):
        if q in skip:
            continue
        assert a[0] == b[0] and a[2] == b[2], (what, q, a, b)
        assert np.array_equal(np.float32(a[3]), np.float32(b[3])), (what, q, a, b)


class Scene:
    """48 queries on make_pair(256, 6, 3), held in a capacity-64 pipeline (with `discs` as the pipeline's footprint), their edges, and the
    world with the wall added (World.update run); nothing has been uploaded after the searches"""

    def __init__(self, discs=None, nearest=False):
        import pathplanning_amd as pa
        self.w, self.ms, self.val, self.ctx = make_pair(256, 6, 3)
        if nearest:
            self.ms.upload_nearest_cells(*O.world_nearest(self.w))
        rng = np.random.RandomState(77)
        if discs is None:
            self.starts, self.goals = valid_random_poses(rng, self.w, N), valid_random_poses(rng, self.w, N)
        else:
            g = R.Grid(self.w)
            self.starts, self.goals = R.valid_poses(rng, g, self.w, N, discs), R.valid_poses(rng, g, self.w, N, discs)
        self.seeds = np.arange(N, dtype=np.uint64) + 1200
        self.pipe = pa.HybridAStarPipeline(self.val, capacity=CAPACITY, max_nodes=32768, search_rows=16)
        self.pipe.initialize()
        self.footprint = None
        if discs is not None:
            self.footprint = pa.Footprint(self.ms, discs)
            self.pipe.set_footprint(self.footprint)
        self.tickets = self.pipe.submit(self.starts, self.goals, self.seeds)
        assert len(self.tickets) == N
        self.got = drain(self.pipe, N)
        self.plans = [self.pipe.get_path_of(t) if self.got[int(t)].status == 0 else None for t in self.tickets]
        self.edges = Edges(self.plans, self.goals, self.ctx)

    def add_wall(self):
        """the wall in the oracle world (not yet on the device)"""
        self.w.add_rectangle(*WALL)
        self.w.update()

    def upload(self, ms):
        ms.upload_dist2(self.w.d2())
        ms.upload_occupancy(self.w.occ())
        ms.upload_path_cost(self.w.pathcost())

    def close(self):
        self.pipe.close()


def mix(results):
    """(blocked plans, still-valid plans)"""
    return sum(r.status == 1 for r in results), sum(r.status == 0 for r in results)


def test_point_validator_on_the_same_map_before_and_after_a_wall():
    """(a) every field equals what pp_check_arcs / pp_check_rs_paths / pp_check_states give for the rebuilt edges, status / edge / ratio equal
    the oracle's, before and after the map gains the wall"""
    s = Scene()
    solved = [p is not None for p in s.plans]
    assert sum(solved) >= 47
    before = s.pipe.revalidate(s.tickets)
    same_exactly(before, s.edges.by_validator(s.val), "unchanged map")
    same_verdict_and_ratio(before, s.edges.by_oracle(s.w), "unchanged map, oracle")
    assert all(r.status == (0 if ok else -1) for r, ok in zip(before, solved))  # on the unchanged map every solved plan is still valid
    assert all(r.valid_length == r.length and r.blocked_edge == 0 and r.blocked_ratio == 1.0 for r in before)
    s.add_wall()
    assert s.pipe.in_flight() == 0
    s.upload(s.ms)
    after = s.pipe.revalidate(s.tickets)
    want = s.edges.by_validator(s.val)
    same_exactly(after, want, "with the wall")
    same_verdict_and_ratio(after, s.edges.by_oracle(s.w), "with the wall, oracle")
    n_blocked, n_valid = mix(after)
    kinds = [(s.plans[q]["kind"][r.blocked_edge], r.blocked_edge) for q, r in enumerate(after) if r.status == 1]
    print("with the wall: %d blocked (%d on an arc, %d on the Reeds-Shepp edge), %d still valid; first blocked edges %s" %
          (n_blocked, sum(k == 1 for k, _ in kinds), sum(k == 2 for k, _ in kinds), n_valid, sorted(e for _, e in kinds)))
    assert n_blocked >= 8 and n_valid >= 8
    assert any(k == 1 for k, _ in kinds) and any(k == 2 for k, _ in kinds)
    for r in after:
        if r.status == 1:
            assert 1 <= r.blocked_edge <= r.n_edges and 0.0 <= r.blocked_ratio < 1.0 and 0.0 <= r.valid_length < r.length
    # an empty call is PP_OK and a subset in another order gives the subset's records
    assert s.pipe.revalidate([]) == []
    pick = [7, 2, 40, 0, 5]
    same_exactly(s.pipe.revalidate([s.tickets[i] for i in pick]), [want[i] for i in pick], "subset")
    s.close()


def test_second_map_with_queries_in_flight_and_processed_paths_kept():
    """(b) the edited grids go into a SECOND map set; revalidate(tickets, map_set=second) runs while a fresh submission is searching the first
    map; the processed paths of an earlier postprocess call stay readable; the in-flight queries end with the batch planner's results"""
    import pathplanning_amd as pa
    import torch
    s = Scene(nearest=True)
    post = s.pipe.postprocess(s.tickets[:6], path_interpolation=0.8)
    paths = s.pipe.get_processed_paths(s.tickets[:6])
    s.add_wall()
    second = pa.OccupancyMapSet.from_bounds(s.ctx, s.w.lb, s.w.ub, 0.1)
    s.upload(second)
    val2 = pa.StateValidatorOccupancyMap(second)
    want = s.edges.by_validator(val2)
    # 8 fresh queries on the first map, the long one (4067 expansions in the oracle: test_gpu_pipeline_postprocess.py) first; from device arrays,
    # so that the submission does not wait for the device
    rng = np.random.RandomState(42)
    s40, g40 = valid_random_poses(rng, s.w, 40), valid_random_poses(rng, s.w, 40)
    fs, fg, fz = np.ascontiguousarray(s40[10:18]), np.ascontiguousarray(g40[10:18]), np.arange(8, dtype=np.uint64) + 910
    batch = pa.HybridAStarBatch(s.val, max_batch=8, max_nodes=32768)
    batch.initialize(s.pipe.nonholo_table())
    ref = batch.search_batch(fs, fg, fz)
    dev = torch.device("cuda", 0)
    d_s, d_g, d_z = torch.from_numpy(fs).to(dev), torch.from_numpy(fg).to(dev), torch.from_numpy(fz.astype(np.int64)).to(dev)
    first, took = s.pipe.submit_dev(d_s, d_g, d_z)
    assert took == 8 and s.pipe.in_flight() == 8
    t0 = time.time()
    got = s.pipe.revalidate(s.tickets, map_set=second)
    print("revalidate of %d held plans beside 8 queries in flight: %.2f ms" % (N, 1e3 * (time.time() - t0)))
    assert s.pipe.in_flight() == 8  # nothing was polled
    same_exactly(got, want, "second map")
    n_blocked, n_valid = mix(got)
    assert n_blocked >= 8 and n_valid >= 8
    # the first map is untouched: on it every solved plan is still valid
    assert all(r.status in (0, -1) for r in s.pipe.revalidate(s.tickets))
    # the last post-processing call's results are still there, and the lengths are the same doubles
    again = s.pipe.get_processed_paths(s.tickets[:6])
    for k in range(6):
        assert np.array_equal(again[k]["sampled"], paths[k]["sampled"]) and np.array_equal(again[k]["smoothed"], paths[k]["smoothed"], equal_nan=True)
        assert again[k]["status"] == paths[k]["status"]
        if post[k].n_points:
            assert got[k].length == post[k].length
    # the queries in flight end as the batch planner's
    fresh = drain(s.pipe, 8)
    for i in range(8):
        r = fresh[first + i]
        assert (r.status, r.n_expanded, r.n_path, r.cost) == (ref[i].status, ref[i].n_expanded, ref[i].n_path, ref[i].cost)
    # ... and the same grids in the pipeline's own map give the same records
    s.upload(s.ms)
    assert as_tuples(s.pipe.revalidate(s.tickets)) == as_tuples(got)
    batch.close()
    s.close()


def test_footprint_equals_the_footprint_entry_points_and_the_restatement():
    """(c) plans searched with a cover_rectangle footprint (4.8 m x 2 m, three discs: the shape of footprint_ref.CAR3): equal to
    pp_check_arcs_footprint / pp_check_rs_paths_footprint / pp_check_states_footprint, and to tests/footprint_ref.py outside its guard band"""
    import pathplanning_amd as pa
    discs = pa.Footprint.rectangle_discs(4.8, 2.0, 1.0, 3)
    s = Scene(discs=discs)
    fp = s.footprint
    assert sum(p is not None for p in s.plans) >= 8

    def compare(what):
        got = s.pipe.revalidate(s.tickets)
        same_exactly(got, s.edges.by_validator(s.val, footprint=fp), what)
        want, guarded = s.edges.by_footprint_ref(R.Grid(s.w), fp.discs)
        left_out = sum(len(s.plans[q]["poses"]) - 1 for q in guarded)
        assert left_out <= R.MAX_LEFT_OUT * s.edges.n_edges, (left_out, s.edges.n_edges)
        same_verdict_and_ratio(got, want, what + ", restatement", skip=guarded)
        return got

    before = compare("footprint, unchanged map")
    assert all(r.status in (0, -1) for r in before)
    s.add_wall()
    s.upload(s.ms)
    after = compare("footprint, with the wall")
    n_blocked, n_valid = mix(after)
    print("footprint, with the wall: %d blocked, %d still valid" % (n_blocked, n_valid))
    assert n_blocked >= 1 and n_valid >= 1
    # the same held plans under the point-disc footprint and under no footprint: the point validator's records both times
    s.pipe.set_footprint(pa.Footprint(s.ms, [(0.0, 0.0, s.val.min_safe_radius)]))
    as_disc = s.pipe.revalidate(s.tickets)
    s.pipe.set_footprint(None)
    as_point = s.pipe.revalidate(s.tickets)
    assert as_tuples(as_disc) == as_tuples(as_point)
    same_exactly(as_point, s.edges.by_validator(s.val), "footprint plans under the point validator")
    s.close()


def test_the_point_disc_gives_the_point_validators_records_bit_for_bit():
    """(c) the scenario of (a) with the footprint {(0, 0, minSafeRadius)} set while the plans are held"""
    import pathplanning_amd as pa
    s = Scene()
    s.add_wall()
    s.upload(s.ms)
    want = as_tuples(s.pipe.revalidate(s.tickets))
    s.pipe.set_footprint(pa.Footprint(s.ms, [(0.0, 0.0, s.val.min_safe_radius)]))  # legal: nothing is in flight, the slots are merely held
    got = s.pipe.revalidate(s.tickets)
    assert as_tuples(got) == want
    assert mix(got)[0] >= 8
    s.close()


def test_a_plan_of_more_than_64_edges_blocked_late():
    """(d) corner to corner on the 1024^2 world: more than 65 poses, so lanes take a second edge and the length is a long sequential sum; a
    rectangle across the plan's 74th edge (placed with the oracle on the CPU) blocks it beyond edge 64"""
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(1024, 24, 1)
    pipe = pa.HybridAStarPipeline(val, capacity=4, max_nodes=65536, search_rows=4)
    pipe.initialize()
    goals = np.array([[48.0, 48.0, 0.0]])
    tickets = pipe.submit([[-48.0, -48.0, 0.0]], goals, [7])
    got = drain(pipe, 1)
    assert got[int(tickets[0])].status == 0 and got[int(tickets[0])].n_path > 65
    plans = [pipe.get_path_of(tickets[0])]
    edges = Edges(plans, goals, ctx)
    before = pipe.revalidate(tickets)
    same_exactly(before, edges.by_validator(val), "long plan")
    same_verdict_and_ratio(before, edges.by_oracle(w), "long plan, oracle")
    assert before[0].status == 0 and before[0].n_edges == got[int(tickets[0])].n_path - 1
    late = plans[0]["poses"][len(plans[0]["poses"]) - 13]  # (pose 74 of the oracle's 87)
    w.add_rectangle(4.0, 0.5, (float(late[0]), float(late[1]), float(late[2]) + np.pi / 2))
    w.update()
    ms.upload_dist2(w.d2())
    after = pipe.revalidate(tickets)
    same_exactly(after, edges.by_validator(val), "long plan, blocked late")
    same_verdict_and_ratio(after, edges.by_oracle(w), "long plan, blocked late, oracle")
    assert after[0].status == 1 and after[0].blocked_edge > 64 and after[0].length == before[0].length
    pipe.close()


def test_a_one_pose_plan_and_a_failed_search():
    """(d) on an open 16 m box with a closed room: a goal inside the room (no plan: -1) and start == goal (one pose, no edge: valid until a
    wall covers the pose, then status 2)"""
    import pathplanning_amd as pa
    lower, upper = (-8.0, -8.0, -np.pi), (8.0, 8.0, np.pi)
    w = O.World(lower=lower, upper=upper, resolution=0.1)
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
    got = drain(pipe, 3)
    assert [got[int(t)].status for t in tickets] == [-1, 0, 0] and got[int(tickets[1])].n_path == 1
    plans = [None] + [pipe.get_path_of(t) for t in tickets[1:]]
    edges = Edges(plans, goals, ctx)
    before = pipe.revalidate(tickets)
    same_exactly(before, edges.by_validator(val), "box")
    assert as_tuples(before)[0] == (-1, 0, 0, 1.0, 0.0, 0.0)
    assert as_tuples(before)[1] == (0, 0, 0, 1.0, 0.0, 0.0)
    assert before[2].status == 0 and before[2].n_edges >= 1
    w.add_rectangle(1.0, 0.3, (-5.0, 3.0, 0.0))
    w.update()
    ms.upload_dist2(w.d2())
    after = pipe.revalidate(tickets)
    same_exactly(after, edges.by_validator(val), "box, a wall on the one-pose plan")
    same_verdict_and_ratio(after, edges.by_oracle(w), "box, oracle")
    assert as_tuples(after)[1] == (2, 0, 0, 1.0, 0.0, 0.0) and after[0].status == -1 and after[2].status == 0
    pipe.close()


def test_refusals_name_the_ticket_and_leave_the_pipeline_usable():
    """(e) every refusal is PP_ERR_INVALID with the first offending ticket named; a valid call afterwards gives the records of before"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError, RevalidateResult, ptr
    s = Scene()
    lib, pipe = s.pipe.lib, s.pipe
    want = as_tuples(pipe.revalidate(s.tickets))
    held = [int(t) for t in s.tickets]
    out = (RevalidateResult * 128)()

    def refused(tickets, *words, n=None, target=None):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        rc = lib.pp_pipeline_revalidate(pipe.h, target, len(t) if n is None else n, ptr(t), out)
        msg = lib.pp_last_error().decode()
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    rng = np.random.RandomState(42)
    s40, g40 = valid_random_poses(rng, s.w, 40), valid_random_poses(rng, s.w, 40)
    flying = pipe.submit(s40[10:11], g40[10:11], np.array([910], dtype=np.uint64))  # a long search (4067 expansions in the oracle)
    assert len(flying) == 1
    with pytest.raises(PPError) as e:
        pipe.revalidate([held[0], int(flying[0]), held[1]])
    assert e.value.code == PP_ERR_INVALID and "ticket %d" % int(flying[0]) in str(e.value) and "in flight" in str(e.value)
    assert pipe.in_flight() == 1  # (it was refused while in flight, not after)
    drain(pipe, 1)
    pipe.release(flying)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "released")
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused((held + held)[:CAPACITY + 1], "capacity")
    refused(held[:1], "capacity", n=-1)
    assert lib.pp_pipeline_revalidate(pipe.h, None, 0, None, out) == 0  # n == 0 is PP_OK
    other = pa.Context(0)
    foreign = pa.OccupancyMapSet.from_bounds(other, s.w.lb, s.w.ub, 0.1)
    foreign.upload_dist2(s.w.d2())
    refused(held[:2], "another context", target=foreign.h)
    bare = pa.OccupancyMapSet.from_bounds(s.ctx, s.w.lb, s.w.ub, 0.1)
    refused(held[:2], "no distance grid", target=bare.h)
    with pytest.raises(PPError):
        pipe.revalidate(held[:2], map_set=bare)
    assert as_tuples(pipe.revalidate(s.tickets)) == want
    s.close()


@pytest.mark.parametrize("with_footprint", [False, True])
def test_the_batch_form_on_a_one_wave_planner(with_footprint):
    """(f) HybridAStarBatch.revalidate: the same kernel with identity slots, against the same comparators, on the planner's own map and on a
    second map"""
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    rng = np.random.RandomState(77)
    fp = pa.Footprint.cover_rectangle(ms, 4.8, 2.0, 1.0, 3) if with_footprint else None
    if with_footprint:
        g = R.Grid(w)
        starts, goals = R.valid_poses(rng, g, w, N, fp.discs), R.valid_poses(rng, g, w, N, fp.discs)
    else:
        starts, goals = valid_random_poses(rng, w, N), valid_random_poses(rng, w, N)
    batch = pa.HybridAStarBatch(val, max_batch=N, max_nodes=32768)  # one wave per query: the planner that takes a footprint
    assert batch.search_rows == 0
    batch.initialize()
    if with_footprint:
        batch.set_footprint(fp)
    res = batch.search_batch(starts, goals, np.arange(N, dtype=np.uint64) + 1200)
    plans = [batch.get_path_of(q) if res[q].status == 0 else None for q in range(N)]
    edges = Edges(plans, goals, ctx)
    before = batch.revalidate()
    same_exactly(before, edges.by_validator(val, footprint=fp), "batch, unchanged map")
    assert all(r.status == (0 if p is not None else -1) for r, p in zip(before, plans))
    w.add_rectangle(*WALL)
    w.update()
    second = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, 0.1)
    second.upload_dist2(w.d2())
    pa.StateValidatorOccupancyMap(second)
    on_second = batch.revalidate(map_set=second)
    assert all(r.status in (0, -1) for r in batch.revalidate(10)) and len(batch.revalidate(10)) == 10  # the planner's own map is untouched
    ms.upload_dist2(w.d2())
    after = batch.revalidate()
    same_exactly(after, edges.by_validator(val, footprint=fp), "batch, with the wall")
    assert as_tuples(on_second) == as_tuples(after)
    if with_footprint:
        want, guarded = edges.by_footprint_ref(R.Grid(w), fp.discs)
        assert sum(len(plans[q]["poses"]) - 1 for q in guarded) <= R.MAX_LEFT_OUT * edges.n_edges
        same_verdict_and_ratio(after, want, "batch, restatement", skip=guarded)
    else:
        same_verdict_and_ratio(after, edges.by_oracle(w), "batch, oracle")
        assert mix(after)[0] >= 8 and mix(after)[1] >= 8
    assert mix(after)[0] >= 1 and mix(after)[1] >= 1
    batch.close()


def test_the_cpp_mirror_revalidates_like_its_path_objects():
    """tests/cpp/test_pipeline_revalidate.cpp: Revalidate(tickets) of Planner::HybridAStarPipeline against HybridAStar::GetGraphSearchPath's
    path objects marched one by one"""
    from pathplanning_amd import build
    exe = build.build_pipeline_revalidate_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"Revalidate(tickets) == the path objects marched one by one" in r.stdout
