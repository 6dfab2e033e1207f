"""-m gpu: held plans stamped into a map's occupancy grid, by ticket (pp_pipeline_stamp, pp_planner_stamp; k_stamp_tickets in
pathplanning_amd/csrc/pp_stamp.hpp; the definition is in include/pp_hip.h).

The comparator is a restatement in numpy that shares nothing with the kernel: every plan's edges are rebuilt from get_path_of as
tests/test_gpu_pipeline_revalidate.py rebuilds them; an edge's length is the plan's own bits; arc poses come from the closed form of
ConstantSteer in numpy, Reeds-Shepp poses from pp_rs_path_interpolate on records built from the plan's word and t, u, v; the discs, the cell
rule and the max-write are plain numpy.

status, n_samples and length must be EQUAL (length to revalidate's).  Cells are compared under an undecided band: with EPS = 1e-7 m a cell
is decided-in if some (sample, disc) has dist <= R - EPS, decided-out if all have dist > R + EPS, undecided otherwise and left out (device and
glibc poses differ around 1e-12 m).  Every decided cell must match exactly, value included.  At most 0.1 % of the restatement's stamped cells
may be undecided per comparison: a band of 2 EPS around a 1 m circle holds about 1e-4 cell centres per disc sample, a few cells in a few
hundred thousand for 48 plans.  cell_box must contain every decided-in cell of its plan and lie inside the box of decided-in + undecided.

World and plans: synthetic_world(256, 14, 3) with the validator (1.0, 0.1) and the query recipe of tests/test_gpu_heuristic_clearance.py
(valid random poses 2i / 2i + 1 of RandomState(7), seed i), 48 of them held in a capacity-64 pipeline, plus one query pair searched twice more
under other seeds.  The pipeline is shared by the tests of this file; every test leaves it without a footprint and with nothing in flight."""
import ctypes as C
import functools
import math
import os
import subprocess
import time

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

N, CAPACITY = 48, 64
RES = 0.1
EPS = 1e-7
MAX_UNDECIDED = 1e-3
MAX_STEPS = 1 << 19
PP_ERR_INVALID = -1
OTHER = dict(lower=(-7.49, -9.74), upper=(7.49, 9.74), resolution=0.15)  # a 100 x 130 grid at 0.15 whose origin (-7.49, -9.74) lies inside the 256^2 world
# which of t, u, v, pi/2 feeds each motion of a Reeds-Shepp word's family (word // 4): reeds_shepp.cpp:306-414
RS_FEED = {0: (0, 1, 2), 1: (0, 1, 2), 2: (0, 1, 2), 3: (0, 1, 2), 4: (0, 1, 2), 5: (0, 1, 1, 2), 6: (0, 1, 1, 2), 7: (0, 3, 1, 2), 8: (0, 3, 1, 2),
           9: (0, 1, 3, 2), 10: (0, 1, 3, 2), 11: (0, 3, 1, 3, 2)}


# ---------------------------------------------------------------------------------------------------- the scene --
def _world():
    w = O.synthetic_world(256, 14, 3)
    w.set_validator(1.0, 0.1)
    return w


def _queries(w, n):
    half = 256 * RES / 2
    rng = np.random.RandomState(7)
    qs = []
    while len(qs) < 2 * n:
        p = np.array([rng.uniform(-half + 1.5, half - 1.5), rng.uniform(-half + 1.5, half - 1.5), rng.uniform(-3.1, 3.1)])
        if w.is_state_valid(p[None])[0]:
            qs.append(p)
    return np.array(qs[0::2]), np.array(qs[1::2]), np.arange(n, dtype=np.uint64)


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


def steps(L, spacing):
    if not L > 0.0:
        return 0
    q = L / spacing
    return MAX_STEPS if not q < MAX_STEPS else int(math.ceil(q))


class Plans:
    """the edges of a list of plans (get_path_of dicts; None = no plan) and their samples, restated"""

    def __init__(self, plans, goals, ctx):
        import pathplanning_amd as pa
        self.plans = plans
        _, self.curv, self.direc = pa.HybridAStarSearchParameters().primitives()
        self.rsp = pa.ReedsSheppPaths(ctx, min_turning_radius=2.0)
        self.rs = {}
        at = [(q, len(p["poses"]) - 1) for q, p in enumerate(plans) if p is not None and len(p["poses"]) > 1 and p["kind"][-1] == 2]
        if at:
            rec = self.rsp.connect(np.array([plans[q]["poses"][e - 1] for q, e in at]), np.array([goals[q] for q, e in at]))
            for i, (q, e) in enumerate(at):
                p = plans[q]
                word, tuv = int(p["prim"][e]), p["tuv"][e]
                assert rec["word"][i] == word and abs(rec["length"][i] - p["length"][e]) < 1e-9
                feed = RS_FEED[word // 4]
                r = rec[i:i + 1].copy()
                for k, f in enumerate(feed):  # the record of the plan's own word and t, u, v (connect() solved the word again: last bits may differ)
                    r["motion_length"][0][k] = (tuv[0], tuv[1], tuv[2], math.pi / 2)[f]
                assert np.abs(r["motion_length"][0][:len(feed)] - rec["motion_length"][i][:len(feed)]).max() < 1e-9
                r["length"][0] = p["length"][e]
                self.rs[q] = r
        self._cache = {}

    def length(self, q):
        total = 0.0
        for e in range(1, len(self.plans[q]["poses"])):
            total = total + float(self.plans[q]["length"][e])
        return total

    def samples(self, q, spacing):
        """(poses [m, 3], arc lengths [m]) of every sample of plan q, edge after edge"""
        if (q, spacing) in self._cache:
            return self._cache[(q, spacing)]
        p = self.plans[q]
        n_path = len(p["poses"])
        if n_path == 1:
            out = (p["poses"][:1].copy(), np.zeros(1))
        else:
            poses, arc, before = [], [], 0.0
            for e in range(1, n_path):
                L = float(p["length"][e])
                n = steps(L, spacing)
                ratio = np.arange(n + 1, dtype=np.float64) / np.float64(n) if n else np.zeros(1)
                arc.append(before + ratio * L)
                if p["kind"][e] == 1:
                    x0, y0, t0 = p["poses"][e - 1]
                    kappa, d = self.curv[int(p["prim"][e])], L * ratio
                    if self.direc[int(p["prim"][e])]:
                        d = -d
                    if abs(kappa) > 1e-9:  # ConstantSteer, kinematic_bicycle_model.cpp:5-32
                        t = t0 + d * kappa
                        poses.append(np.column_stack([x0 + 1 / kappa * (np.sin(t) - math.sin(t0)), y0 + 1 / kappa * (-np.cos(t) + math.cos(t0)), t]))
                    else:
                        poses.append(np.column_stack([x0 + d * math.cos(t0), y0 + d * math.sin(t0), np.full(len(d), t0)]))
                else:
                    assert p["kind"][e] == 2 and e == n_path - 1
                    poses.append(self.rsp.interpolate(np.repeat(self.rs[q], len(ratio)), ratio)[0])
                before = before + L
            out = (np.concatenate(poses), np.concatenate(arc))
        self._cache[(q, spacing)] = out
        return out


class Geometry:
    def __init__(self, ms):
        self.rows, self.cols, self.res = ms.rows, ms.cols, float(np.float32(ms.resolution))
        self.gx, self.gy = float(ms.grid_origin[0]), float(ms.grid_origin[1])


def rasterise(g, centres, R):
    """(decided-in mask, band mask) of discs of radius R at `centres` [m, 2] on geometry g"""
    inn, band = np.zeros((g.rows, g.cols), dtype=bool), np.zeros((g.rows, g.cols), dtype=bool)
    off = np.arange(-(int(math.ceil(R / g.res)) + 2), int(math.ceil(R / g.res)) + 3)
    for k in range(0, len(centres), 4096):
        c = centres[k:k + 4096]
        r = np.floor((c[:, 0] - g.gx) / g.res).astype(np.int64)[:, None] + off[None, :]
        cl = np.floor((c[:, 1] - g.gy) / g.res).astype(np.int64)[:, None] + off[None, :]
        dx = (g.gx + (r + 0.5) * g.res) - c[:, 0, None]
        dy = (g.gy + (cl + 0.5) * g.res) - c[:, 1, None]
        d = np.sqrt(dx[:, :, None] ** 2 + dy[:, None, :] ** 2)
        ok = ((r >= 0) & (r < g.rows))[:, :, None] & ((cl >= 0) & (cl < g.cols))[:, None, :]
        rr, cc = np.broadcast_to(r[:, :, None], d.shape), np.broadcast_to(cl[:, None, :], d.shape)
        a = ok & (d <= R - EPS)
        b = ok & ~a & (d <= R + EPS)
        inn[rr[a], cc[a]] = True
        band[rr[b], cc[b]] = True
    return inn, band & ~inn


def box_of(mask):
    if not mask.any():
        return None
    r, c = np.nonzero(mask)
    return r.min(), r.max(), c.min(), c.max()


def expect(P, order, g, discs, margin, spacing, values=None, lo=None, hi=None, before=None):
    """the restatement of one stamp call over plans `order` (indices into P.plans): (records, grid, undecided mask, stamped cells)"""
    grid = np.full((g.rows, g.cols), -1, dtype=np.int32) if before is None else before.copy()
    undecided = np.zeros((g.rows, g.cols), dtype=bool)
    stamped = np.zeros((g.rows, g.cols), dtype=bool)
    records = []
    for i, q in enumerate(order):
        if P.plans[q] is None or len(P.plans[q]["poses"]) == 0:
            records.append(dict(status=-1, n_samples=0, length=0.0, inn=None, band=None))
            continue
        poses, arc = P.samples(q, spacing)
        keep = (arc >= (-np.inf if lo is None else lo[i])) & (arc <= (np.inf if hi is None else hi[i]))
        poses = poses[keep]
        inn, band = np.zeros((g.rows, g.cols), dtype=bool), np.zeros((g.rows, g.cols), dtype=bool)
        for ox, oy, r in discs:
            if ox == 0.0 and oy == 0.0:
                centres = poses[:, :2]
            else:
                s, c = np.sin(poses[:, 2]), np.cos(poses[:, 2])
                centres = np.column_stack([(poses[:, 0] + ox * c) - oy * s, (poses[:, 1] + ox * s) + oy * c])
            a, b = rasterise(g, centres, float(np.float32(r)) + float(np.float32(margin)))
            inn |= a
            band |= b
        band &= ~inn
        v = 0 if values is None else int(values[i])
        grid[inn] = np.maximum(grid[inn], v)
        undecided |= band
        stamped |= inn
        records.append(dict(status=0, n_samples=int(keep.sum()), length=P.length(q), inn=inn, band=band))
    return records, grid, undecided, stamped


def compare(got, device_grid, want, what, lengths=None):
    records, grid, undecided, stamped = want
    assert len(got) == len(records)
    for i, (a, b) in enumerate(zip(got, records)):
        print("%s plan %2d: status %d samples %d box %s length %.17g | want status %d samples %d" %
              (what, i, a.status, a.n_samples, tuple(a.cell_box), a.length, b["status"], b["n_samples"]))
        assert (a.status, a.n_samples) == (b["status"], b["n_samples"]) and a.length == b["length"], (what, i)
        if lengths is not None:
            assert a.length == lengths[i], (what, i)
        box = tuple(a.cell_box)
        if b["status"] != 0:
            assert box[0] > box[1]
            continue
        inner, outer = box_of(b["inn"]), box_of(b["inn"] | b["band"])
        if outer is None:
            assert box[0] > box[1], (what, i, box)
        if inner is not None:
            assert box[0] <= inner[0] and box[1] >= inner[1] and box[2] <= inner[2] and box[3] >= inner[3], (what, i, box, inner)
        if box[0] <= box[1]:
            assert outer is not None and box[0] >= outer[0] and box[1] <= outer[1] and box[2] >= outer[2] and box[3] <= outer[3], (what, i, box, outer)
    n_undecided, n_stamped = int(undecided.sum()), int(stamped.sum())
    print("%s: %d cells stamped, %d undecided" % (what, n_stamped, n_undecided))
    assert n_undecided <= MAX_UNDECIDED * n_stamped, (what, n_undecided, n_stamped)
    decided = ~undecided
    bad = np.argwhere(decided & (device_grid != grid))
    assert len(bad) == 0, (what, len(bad), bad[:5], device_grid[tuple(bad[0])], grid[tuple(bad[0])])
    return n_stamped


class Scene:
    def __init__(self):
        import pathplanning_amd as pa
        self.w = _world()
        self.ctx = pa.Context(0)
        self.ms = self.fresh(upload=True)
        self.val = pa.StateValidatorOccupancyMap(self.ms)
        self.starts, self.goals, self.seeds = _queries(self.w, N)
        # + query 3's pair twice more under other seeds: plans of one start / goal that differ
        self.starts = np.concatenate([self.starts, self.starts[3:4], self.starts[3:4]])
        self.goals = np.concatenate([self.goals, self.goals[3:4], self.goals[3:4]])
        self.seeds = np.concatenate([self.seeds, np.array([1003, 2003], dtype=np.uint64)])
        self.pipe = pa.HybridAStarPipeline(self.val, capacity=CAPACITY, max_nodes=32768, search_rows=16)
        self.pipe.initialize()
        self.all_tickets = self.pipe.submit(self.starts, self.goals, self.seeds)
        assert len(self.all_tickets) == N + 2
        self.got = drain(self.pipe, N + 2)
        self.plans = [self.pipe.get_path_of(t) if self.got[int(t)].status == 0 else None for t in self.all_tickets]
        self.P = Plans(self.plans, self.goals, self.ctx)
        self.tickets = self.all_tickets[:N]
        self.point = [(0.0, 0.0, float(self.val.min_safe_radius))]
        self.lengths = [r.length for r in self.pipe.revalidate(self.all_tickets)]

    def fresh(self, upload=False, other=False, shifted=False):
        """a map set of the context: the world's geometry (with the world's grids if `upload`), or the OTHER geometry, bare, or -- shifted -- a
        100 x 130 grid at 0.15 m with its origin at (-1, -9): it leaves out the world's left part, where whole plans lie"""
        import pathplanning_amd as pa
        if shifted:
            return pa.OccupancyMapSet(self.ctx, (-1.0, -9.0, -math.pi), (14.0, 10.5, math.pi), 0.15, 100, 130, (-1.0, -9.0))
        if other:
            w2 = O.World(**OTHER)
            ms = pa.OccupancyMapSet.from_bounds(self.ctx, w2.lb, w2.ub, OTHER["resolution"])
            assert (ms.rows, ms.cols) == (w2.rows, w2.cols) == (100, 130) and np.array_equal(ms.grid_origin, w2.origin)
            return ms
        ms = pa.OccupancyMapSet.from_bounds(self.ctx, self.w.lb, self.w.ub, RES)
        assert (ms.rows, ms.cols) == (self.w.rows, self.w.cols)
        if upload:
            ms.upload_dist2(self.w.d2())
            ms.upload_occupancy(self.w.occ())
            ms.upload_path_cost(self.w.pathcost())
        return ms


@functools.lru_cache(maxsize=None)
def scene():
    return Scene()


def test_the_scene_has_arcs_and_reeds_shepp_edges():
    s = scene()
    solved = [p for p in s.plans[:N] if p is not None]
    assert len(solved) >= 40
    assert any((p["kind"][1:] == 1).any() for p in solved) and sum(p["kind"][-1] == 2 for p in solved) >= 20
    assert s.plans[N] is not None and s.plans[N + 1] is not None  # (the two seeds may well give one and the same plan: test_values does not need them to differ)


# ------------------------------------------------------------------------------------------------------ 1, 2 --
def test_whole_plans_into_the_same_and_into_another_geometry():
    """(1) no footprint, margin 0: a second map of the same geometry (which has no occupancy grid yet), then the 100 x 130 target at 0.15 m,
    where most plans are clipped and some miss: status 0, samples counted, an empty box"""
    s = scene()
    order = list(range(N))
    B = s.fresh()
    got = s.pipe.stamp(s.tickets, map_set=B, spacing=0.1)
    n = compare(got, B.download_occupancy(), expect(s.P, order, Geometry(B), s.point, 0.0, 0.1), "same geometry", s.lengths[:N])
    assert n > 10000
    Cm = s.fresh(shifted=True)
    got = s.pipe.stamp(s.tickets, map_set=Cm, spacing=0.1)
    want = expect(s.P, order, Geometry(Cm), s.point, 0.0, 0.1)
    compare(got, Cm.download_occupancy(), want, "other geometry", s.lengths[:N])
    boxes = [tuple(r.cell_box) for r in got if r.status == 0]
    missed = [b for b in boxes if b[0] > b[1]]
    clipped = [b for b in boxes if b[0] <= b[1] and (b[0] == 0 or b[1] == 99 or b[2] == 0 or b[3] == 129)]
    print("other geometry: %d plans miss the target, %d are clipped at its border" % (len(missed), len(clipped)))
    assert len(missed) >= 1 and len(clipped) >= 5
    assert all(r.n_samples > 0 for r in got if r.status == 0)
    # the pipeline's own map was never the target
    assert np.array_equal(s.ms.download_occupancy(), s.w.occ())


@pytest.mark.parametrize("spacing", [0.1, 0.37])
def test_three_disc_footprint_with_a_margin(spacing):
    """(2) pp_footprint_cover_rectangle(4.0, 1.8, 1.0, 3), margin 0.12; at 0.37 an edge holds a fractional number of steps"""
    import pathplanning_amd as pa
    s = scene()
    discs = pa.Footprint.rectangle_discs(4.0, 1.8, 1.0, 3)
    fp = pa.Footprint(s.ms, discs)
    s.pipe.set_footprint(fp)
    try:
        B = s.fresh()
        got = s.pipe.stamp(s.tickets, map_set=B, spacing=spacing, margin=0.12)
        compare(got, B.download_occupancy(), expect(s.P, list(range(N)), Geometry(B), fp.discs, 0.12, spacing), "footprint, spacing %g" % spacing, s.lengths[:N])
        if spacing == 0.37:
            assert any(steps(float(p["length"][1]), spacing) * spacing != float(p["length"][1]) for p in s.plans[:N] if p is not None and len(p["poses"]) > 1)
    finally:
        s.pipe.set_footprint(None)


# ---------------------------------------------------------------------------------------------------------- 3 --
def test_windows():
    """(3) [0.4, 0.7] of the length per ticket (cutting inside edges); from > length and to < 0 (no samples, the grid unchanged); a window
    that holds a single junction pose (sampled twice: the end of one edge and the start of the next)"""
    s = scene()
    order = list(range(N))
    L = np.array(s.lengths[:N])
    B = s.fresh(upload=True)
    lo, hi = 0.4 * L, 0.7 * L
    got = s.pipe.stamp(s.tickets, map_set=B, from_length=lo, to_length=hi, spacing=0.1, values=3)
    want = expect(s.P, order, Geometry(B), s.point, 0.0, 0.1, values=[3] * N, lo=lo, hi=hi, before=s.w.occ())
    compare(got, B.download_occupancy(), want, "window 0.4 .. 0.7", s.lengths[:N])
    whole = expect(s.P, order, Geometry(B), s.point, 0.0, 0.1)[0]
    assert all(a.n_samples < b["n_samples"] for a, b in zip(got, whole) if b["status"] == 0 and b["n_samples"] > 3)
    held = B.download_occupancy()
    for what, a, b in (("from > length", L + 0.5, None), ("to < 0", None, np.full(N, -1e-9))):
        got = s.pipe.stamp(s.tickets, map_set=B, from_length=a, to_length=b, spacing=0.1, values=9)
        assert all(r.n_samples == 0 and r.cell_box[0] > r.cell_box[1] and r.status in (0, -1) for r in got), what
        assert [r.length for r in got] == s.lengths[:N]
        assert np.array_equal(B.download_occupancy(), held), what
    # the junction of edges 1 and 2: s = the first edge's length, exactly
    multi = [q for q in order if s.plans[q] is not None and len(s.plans[q]["poses"]) >= 3]
    at = np.array([float(s.plans[q]["length"][1]) for q in multi])
    D = s.fresh()
    got = s.pipe.stamp([s.tickets[q] for q in multi], map_set=D, from_length=at, to_length=at, spacing=0.1)
    want = expect(s.P, multi, Geometry(D), s.point, 0.0, 0.1, lo=at, hi=at)
    compare(got, D.download_occupancy(), want, "one junction pose")
    assert all(r.n_samples == 2 for r in got)


# ---------------------------------------------------------------------------------------------------------- 4 --
def test_a_plan_of_more_than_64_edges_an_edge_of_more_than_64_samples_and_a_one_pose_plan():
    """(4) corner to corner on the 1024^2 world (87 poses in the oracle: lanes take a second edge in the prologue), at spacing 0.05 (the final
    Reeds-Shepp edge has more than 64 samples: one edge spans several rounds of 64); start == goal (one pose, one sample at s = 0)"""
    import pathplanning_amd as pa
    from gpu_common import make_pair
    w, ms, val, ctx = make_pair(1024, 24, 1)
    pipe = pa.HybridAStarPipeline(val, capacity=4, max_nodes=65536, search_rows=4)
    pipe.initialize()
    goals = np.array([[48.0, 48.0, 0.0], [-48.0, -48.0, 0.0]])
    tickets = pipe.submit([[-48.0, -48.0, 0.0], [-48.0, -48.0, 0.0]], goals, [7, 8])
    got = drain(pipe, 2)
    assert got[int(tickets[0])].status == 0 and got[int(tickets[0])].n_path > 65 and got[int(tickets[1])].n_path == 1
    plans = [pipe.get_path_of(t) for t in tickets]
    P = Plans(plans, goals, ctx)
    lengths = [r.length for r in pipe.revalidate(tickets)]
    point = [(0.0, 0.0, float(val.min_safe_radius))]
    B = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, 0.1)
    for spacing in (0.1, 0.05):
        res = pipe.stamp(tickets, map_set=B, spacing=spacing, values=[spacing == 0.05, 2])
        before = None if spacing == 0.1 else grid
        grid = B.download_occupancy()
        compare(res, grid, expect(P, [0, 1], Geometry(B), point, 0.0, spacing, values=[spacing == 0.05, 2], before=before), "long plan, spacing %g" % spacing, lengths)
        assert res[1].n_samples == 1 and res[1].length == 0.0
    assert max(steps(float(l), 0.05) for l in plans[0]["length"][1:]) > 64
    pipe.close()


# ---------------------------------------------------------------------------------------------------------- 5 --
def test_values():
    """(5) two plans of one query pair with values 5 and 9 give 9 where they overlap, in either ticket order; a target pre-loaded with the
    world's obstacle ids keeps larger ids and loses -1 only where covered; a target without an occupancy grid gets one"""
    s = scene()
    pair = [N, N + 1]
    grids = []
    for order, values in ((pair, [5, 9]), (pair[::-1], [9, 5])):
        B = s.fresh()
        got = s.pipe.stamp([s.all_tickets[q] for q in order], map_set=B, values=values, spacing=0.1)
        want = expect(s.P, order, Geometry(B), s.point, 0.0, 0.1, values=values)
        grids.append(B.download_occupancy())
        compare(got, grids[-1], want, "values %s" % values)
        both = want[0][0]["inn"] & want[0][1]["inn"] & ~want[2]
        assert both.sum() > 100 and (grids[-1][both] == 9).all()
    assert np.array_equal(grids[0], grids[1])
    # ... and with the 9 confined to the first half of its plan, cells that only the 5 covers keep the 5
    half = 0.5 * s.lengths[N + 1]
    for order, values, hi in ((pair, [5, 9], [np.inf, half]), (pair[::-1], [9, 5], [half, np.inf])):
        B = s.fresh()
        got = s.pipe.stamp([s.all_tickets[q] for q in order], map_set=B, values=values, to_length=hi, spacing=0.1)
        want = expect(s.P, order, Geometry(B), s.point, 0.0, 0.1, values=values, hi=hi)
        grids.append(B.download_occupancy())
        compare(got, grids[-1], want, "values %s, the 9 up to %.3f m" % (values, half))
        assert (grids[-1] == 9).sum() > 100 and (grids[-1] == 5).sum() > 100
    assert np.array_equal(grids[2], grids[3])
    occ = s.w.occ()
    assert occ.max() >= 10
    B = s.fresh(upload=True)
    got = s.pipe.stamp(s.tickets, map_set=B, values=6, spacing=0.1, margin=0.3)
    after = B.download_occupancy()
    want = expect(s.P, list(range(N)), Geometry(B), s.point, 0.3, 0.1, values=[6] * N, before=occ)
    compare(got, after, want, "over the world's ids")
    covered = want[3] & ~want[2]
    assert ((occ > 6) & covered).sum() > 0 and np.array_equal(after[(occ > 6) & covered], occ[(occ > 6) & covered])
    assert (after[covered] >= 6).all() and np.array_equal(after[~want[3] & ~want[2]], occ[~want[3] & ~want[2]])
    bare = s.fresh()
    with pytest.raises(Exception):
        bare.download_occupancy()  # no grid yet
    s.pipe.stamp(s.tickets[:1], map_set=bare, spacing=0.1)
    assert 30000 < (bare.download_occupancy() == -1).sum() < 65536


# ---------------------------------------------------------------------------------------------------------- 6 --
def test_beside_queries_in_flight():
    """(6) eight queries submitted on the pipeline's map and not polled; the stamp into map B runs beside them and matches the restatement; the
    queries then complete with the batch planner's results"""
    import pathplanning_amd as pa
    s = scene()
    fs, fg, fz = np.ascontiguousarray(s.goals[:8]), np.ascontiguousarray(s.starts[:8]), np.arange(8, dtype=np.uint64) + 900
    batch = pa.HybridAStarBatch(s.val, max_batch=8, max_nodes=32768)
    batch.initialize(s.pipe.nonholo_table())
    ref = batch.search_batch(fs, fg, fz)
    flying = s.pipe.submit(fs, fg, fz)
    assert len(flying) == 8 and s.pipe.in_flight() == 8
    B = s.fresh()
    t0 = time.time()
    got = s.pipe.stamp(s.tickets, map_set=B, spacing=0.1)
    print("stamp of %d held plans beside 8 queries in flight: %.2f ms" % (N, 1e3 * (time.time() - t0)))
    assert s.pipe.in_flight() == 8  # nothing was polled
    compare(got, B.download_occupancy(), expect(s.P, list(range(N)), Geometry(B), s.point, 0.0, 0.1), "beside queries in flight", s.lengths[:N])
    fresh = drain(s.pipe, 8)
    for i, t in enumerate(flying):
        r = fresh[int(t)]
        assert (r.status, r.n_expanded, r.n_path, r.cost) == (ref[i].status, ref[i].n_expanded, ref[i].n_path, ref[i].cost)
    s.pipe.release(flying)
    batch.close()


# ---------------------------------------------------------------------------------------------------------- 7 --
def blocked_mask(d2, occ, radius, resolution):
    """occupied, or !(dist >= radius) with the map's float distance (gvd.h:38: double sqrt times the float resolution, as float)"""
    dist = (np.sqrt(d2.astype(np.float64)) * np.float64(np.float32(resolution))).astype(np.float32)
    return (occ >= 0) | ~(dist >= np.float32(radius))


def test_the_fields_and_the_clearance_views_follow():
    """(7) after a stamp the exact transform builds the fields from the stamped grid: d2 == 0 exactly on the occupied cells and pp_check_states
    rejects a pose on a stamped cell's centre that it accepted before; after a SECOND stamp, with the distance grid left as it was, the field of
    pp_obstacle_heuristic_clearance equals the oracle's on the downloaded occupancy and squared distances"""
    import pathplanning_amd as pa
    s = scene()
    B = s.fresh(upload=True)
    valB = pa.StateValidatorOccupancyMap(B)
    first, second = s.tickets[:24], s.tickets[24:]
    s.pipe.stamp(first, map_set=B, values=40, spacing=0.1)
    occ = B.download_occupancy()
    new = np.argwhere((occ == 40) & (s.w.d2() >= 400))  # stamped cells 2 m and more from the world's obstacles
    assert len(new) > 100
    r, c = new[len(new) // 2]
    pose = np.array([[B.grid_origin[0] + (r + 0.5) * RES, B.grid_origin[1] + (c + 0.5) * RES, 0.3]])
    assert valB.is_state_valid(pose)[0]  # the distance grid has not followed yet
    B.update_gvd()
    g = B.download_gvd()
    assert np.array_equal(g["d2"] == 0, occ >= 0)
    assert not valB.is_state_valid(pose)[0]
    s.pipe.stamp(second, map_set=B, values=41, spacing=0.1)
    occ2 = B.download_occupancy()
    assert (occ2 == 41).sum() > 1000 and np.array_equal(B.download_gvd()["d2"], g["d2"])  # the fields are the caller's to update
    radius = 0.35
    goal = (float(pose[0, 0]) + 3.0 * RES * (1 if pose[0, 0] < 0 else -1), float(pose[0, 1]))
    free = np.argwhere(~blocked_mask(g["d2"], occ2, radius, RES))
    goals = [goal, (B.grid_origin[0] + (free[len(free) // 3][0] + 0.5) * RES, B.grid_origin[1] + (free[len(free) // 3][1] + 0.5) * RES)]
    got = pa.ObstaclesHeuristic(B).update(goals, clearance=radius)
    w = _world()
    inflated = np.where(blocked_mask(g["d2"], occ2, radius, RES), 0, -1).astype(np.int32)
    inflated[occ2 >= 0] = occ2[occ2 >= 0]
    w.set_occ(inflated)
    w.set_d2(g["d2"])
    for i, xy in enumerate(goals):
        want = w.obstacle_heuristic(xy)[0]
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), i
    assert np.isfinite(got[1]).sum() > 1000


def test_a_reference_order_update_after_a_stamp_reseeds_from_the_grid():
    """(7) the cells a stamp writes are unknown to the ordered edit record: a PP_GVD_REFERENCE_ORDER update afterwards equals the oracle's
    brushfire seeded from the downloaded occupancy, every occupied cell in row-major order -- although the device ran that mode incrementally
    before the stamp"""
    from gpu_common import rect_vertices
    s = scene()
    Cm = s.fresh(other=True)
    w2 = O.World(**OTHER)
    rect = (4.0, 0.6, [1.0, -2.0, 0.4])
    assert w2.add_rectangle(*rect) == 0
    Cm.add_polygon(rect_vertices(rect[0], rect[1]), rect[2], 0)
    w2.update()
    Cm.update_gvd(mode=Cm.GVD_REFERENCE_ORDER)
    assert np.array_equal(Cm.download_gvd()["d2"], w2.d2())
    pick = [q for q in range(N) if s.plans[q] is not None][:12]
    got = s.pipe.stamp([s.tickets[q] for q in pick], map_set=Cm, values=np.arange(len(pick)) % 3 + 1, spacing=0.15)
    assert sum(r.cell_box[0] <= r.cell_box[1] for r in got) >= 3
    occ = Cm.download_occupancy()
    assert (occ > 0).sum() > 500 and (occ == 0).sum() > 10
    Cm.update_gvd(mode=Cm.GVD_REFERENCE_ORDER)
    g = Cm.download_gvd()
    w3 = O.World(**OTHER)
    lib = O.lib()
    zero = np.zeros(3)
    for r, c in np.argwhere(occ >= 0):  # SetObstacle, cell by cell, row-major (a one-vertex outline is one cell)
        xy = np.array([w3.origin[0] + (r + 0.5) * OTHER["resolution"], w3.origin[1] + (c + 0.5) * OTHER["resolution"]])
        lib.ppo_world_add_polygon(w3.h, C.c_int(1), C.c_void_p(xy.ctypes.data), C.c_void_p(zero.ctypes.data))
    assert np.array_equal(w3.occ() >= 0, occ >= 0)
    w3.set_occ(occ)
    w3.update()
    no, ne = O.world_nearest(w3)
    assert np.array_equal(g["d2"], w3.d2()) and np.array_equal(g["nearest_obstacle"], no)
    assert np.array_equal(g["voronoi_d2"], w3.voro_d2()) and np.array_equal(g["nearest_edge"], ne)
    assert np.array_equal(g["path_cost"].view(np.uint32), w3.pathcost().view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- 8 --
def test_refusals_launch_nothing_write_nothing_and_leave_the_pipeline_usable():
    """(8) every refusal is PP_ERR_INVALID with the first offending ticket or argument named; the target's grid and a clearance field over it
    are what they were; a valid call afterwards gives the records of before; n == 0 is PP_OK and touches nothing"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PPError, StampParams, StampResult, ptr
    s = scene()
    lib, pipe = s.pipe.lib, s.pipe
    B = s.fresh(upload=True)
    held = [int(t) for t in s.tickets]
    first = pipe.stamp(held[:6], map_set=B, spacing=0.1, values=2)
    grid = B.download_occupancy()
    goal = [(0.3, -0.2)]
    field = pa.ObstaclesHeuristic(B).update(goal, clearance=0.35)
    out = (StampResult * 128)()
    good = StampParams(0.1, 0.0, 0)

    def refused(tickets, *words, n=None, target=B.h, values=None, lo=None, hi=None, params=good):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        v = None if values is None else np.ascontiguousarray(values, dtype=np.int32)
        a = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
        b = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
        rc = lib.pp_pipeline_stamp(pipe.h, target, len(t) if n is None else n, ptr(t), ptr(v), ptr(a), ptr(b), C.byref(params) if params is not None else None, out)
        msg = lib.pp_last_error().decode()
        print(rc, msg)
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    refused((held + held)[:CAPACITY + 1], "capacity")
    refused(held[:1], "capacity", n=-1)
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused(held[:2], "params", params=None)
    for spacing in (0.0, -0.1, float("nan"), float("inf")):
        refused(held[:2], "spacing", params=StampParams(spacing, 0.0, 0))
    for margin in (-0.01, float("nan"), float("inf")):
        refused(held[:2], "margin", params=StampParams(0.1, margin, 0))
    refused(held[:3], "ticket %d" % held[1], "negative", values=[0, -1, -2])
    refused(held[:3], "ticket %d" % held[2], "NaN", lo=[0.0, 1.0, float("nan")])
    refused(held[:3], "ticket %d" % held[0], "NaN", hi=[float("nan"), 1.0, 2.0])
    other = pa.Context(0)
    foreign = pa.OccupancyMapSet.from_bounds(other, s.w.lb, s.w.ub, RES)
    refused(held[:2], "another context", target=foreign.h)
    # a query in flight: its ticket is refused, and so is the pipeline's OWN map as the target (explicitly or as NULL); another map is not
    flying = pipe.submit(s.goals[8:9], s.starts[8:9], np.array([950], dtype=np.uint64))
    assert len(flying) == 1 and pipe.in_flight() == 1
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "in flight")
    refused(held[:2], "own map", "in flight", target=None)
    refused(held[:2], "own map", "in flight", target=s.ms.h)
    with pytest.raises(PPError) as e:
        pipe.stamp(held[:2], spacing=0.1)
    assert e.value.code == PP_ERR_INVALID
    assert pipe.in_flight() == 1
    drain(pipe, 1)
    pipe.release(flying)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "released")
    assert np.array_equal(s.ms.download_occupancy(), s.w.occ())
    # n == 0, and everything is as it was
    assert lib.pp_pipeline_stamp(pipe.h, B.h, 0, None, None, None, None, C.byref(good), out) == 0
    assert pipe.stamp([], map_set=B) == []
    assert np.array_equal(B.download_occupancy(), grid)
    assert np.array_equal(pa.ObstaclesHeuristic(B).update(goal, clearance=0.35).view(np.uint32), field.view(np.uint32))
    again = pipe.stamp(held[:6], map_set=B, spacing=0.1, values=2)
    assert [(r.status, r.n_samples, tuple(r.cell_box), r.length) for r in again] == [(r.status, r.n_samples, tuple(r.cell_box), r.length) for r in first]
    assert np.array_equal(B.download_occupancy(), grid)
    # with nothing in flight the pipeline's own map is a legal target
    own = pipe.stamp(held[:1], spacing=0.1, from_length=[1e9])
    assert own[0].n_samples == 0 and np.array_equal(s.ms.download_occupancy(), s.w.occ())


# ---------------------------------------------------------------------------------------------------------- 9 --
@pytest.mark.parametrize("with_footprint", [False, True])
def test_the_batch_form_on_a_one_wave_planner(with_footprint):
    """(9) HybridAStarBatch.stamp: the same kernel with identity slots and the planner's footprint, against the same restatement; a planner that is
    a pipeline's buffer set is refused"""
    import pathplanning_amd as pa
    from pathplanning_amd._lib import StampParams, StampResult
    s = scene()
    n = 16
    batch = pa.HybridAStarBatch(s.val, max_batch=n, max_nodes=32768)
    assert batch.search_rows == 0
    batch.initialize(s.pipe.nonholo_table())
    discs = s.point
    if with_footprint:
        fp = pa.Footprint.cover_rectangle(s.ms, 4.0, 1.8, 1.0, 3)
        batch.set_footprint(fp)
        discs = fp.discs
    res = batch.search_batch(s.starts[:n], s.goals[:n], s.seeds[:n])
    plans = [batch.get_path_of(q) if res[q].status == 0 else None for q in range(n)]
    assert sum(p is not None for p in plans) >= 4
    P = Plans(plans, s.goals[:n], s.ctx)
    lengths = [r.length for r in batch.revalidate()]
    B = s.fresh()
    values = np.arange(n) % 4
    got = batch.stamp(map_set=B, values=values, spacing=0.2, margin=0.05)
    compare(got, B.download_occupancy(), expect(P, list(range(n)), Geometry(B), discs, 0.05, 0.2, values=values), "batch form", lengths)
    got = batch.stamp(5, map_set=B, spacing=0.2, from_length=1.0, to_length=3.0, values=7)
    assert len(got) == 5
    out = (StampResult * 4)()
    rc = s.pipe.lib.pp_planner_stamp(s.pipe.planner_h, B.h, 1, None, None, None, C.byref(StampParams(0.1, 0.0, 0)), out)
    assert rc == PP_ERR_INVALID and "pp_pipeline_stamp" in s.pipe.lib.pp_last_error().decode()
    batch.close()


def test_the_cpp_mirror_stamps_like_its_path_objects():
    """tests/cpp/test_pipeline_stamp.cpp: Stamp(tickets) of Planner::HybridAStarPipeline against HybridAStar::GetGraphSearchPath's path objects sampled
    and rasterised one by one"""
    from pathplanning_amd import build
    exe = build.build_pipeline_stamp_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"Stamp(tickets) == the path objects sampled and rasterised one by one" in r.stdout
