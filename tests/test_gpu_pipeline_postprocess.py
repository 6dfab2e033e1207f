"""-m gpu: HybridAStar::SearchPath's post-processing by ticket in the streaming pipeline (pp_pipeline_postprocess,
pp_pipeline_get_processed_paths; k_postprocess_tickets in pathplanning_amd/csrc/pp_postprocess.hpp).  The expected values come from code the
new kernel shares nothing with at run time: the batch planner's k_postprocess on the same queries (bit for bit), the CPU oracle's
restatement of the reference (within the tolerances of test_gpu_postprocess.py at 0.8 m), and for the footprint verdict the validator's
check_states entry, itself pinned to numpy in test_gpu_footprint.py.  256^2 map, 0.8 m spacing, capacity 16, 8 search rows."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import footprint_ref as R
import oracle_lib as O
from gpu_common import make_pair, valid_random_poses

pytestmark = pytest.mark.gpu

SPACING = 0.8
PICK = [7, 2, 10, 0, 5]  # positions in the submission = field slots: not in slot order
PP_ERR_INVALID = -1      # include/pp_hip.h


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


def same_processed(a, b):
    """a pipeline result against a batch-planner result of the same query, as the held-slot test compares, plus the scalars"""
    assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["length"] == b["length"], (a["status"], b["status"], a["iterations"], b["iterations"])
    assert np.array_equal(a["sampled"], b["sampled"]) and np.array_equal(a["cusp"], b["cusp"])
    assert np.array_equal(a["path"], b["path"], equal_nan=True) and np.array_equal(a["smoothed"], b["smoothed"], equal_nan=True)


class Case1:
    """12 queries held in a capacity-16 pipeline, the batch planner's post-processing of the same 12 as the reference; shared by the
    subset test and the refusal test (which ends on the subset's results)"""

    def __init__(self):
        import pathplanning_amd as pa
        self.w, self.ms, self.val, self.ctx = make_pair(256, 6, 3)
        self.ms.upload_nearest_cells(*O.world_nearest(self.w))
        rng = np.random.RandomState(31)
        self.n = n = 12
        self.starts, self.goals = valid_random_poses(rng, self.w, n), valid_random_poses(rng, self.w, n)
        self.seeds = np.arange(n, dtype=np.uint64) + 300
        self.pipe = pa.HybridAStarPipeline(self.val, capacity=16, max_nodes=32768, search_rows=8)
        self.pipe.initialize()
        self.batch = pa.HybridAStarBatch(self.val, max_batch=n, max_nodes=32768)
        self.batch.initialize(self.pipe.nonholo_table())
        self.ref = self.batch.search_batch(self.starts, self.goals, self.seeds)
        self.batch.postprocess(n, path_interpolation=SPACING)
        self.tickets = self.pipe.submit(self.starts, self.goals, self.seeds)
        assert len(self.tickets) == n
        self.got = drain(self.pipe, n)
        for i, t in enumerate(self.tickets):
            assert self.pipe.lib.pp_pipeline_slot_of(self.pipe.h, C.c_uint64(int(t))) == i  # a fresh pipeline hands slot 0 out first
            assert self.got[int(t)].status == self.ref[i].status and self.got[int(t)].n_expanded == self.ref[i].n_expanded

    def check_subset(self):
        """post-processes PICK and compares with the batch planner; returns the processed paths"""
        chosen = [self.tickets[i] for i in PICK]
        post = self.pipe.postprocess(chosen, path_interpolation=SPACING)
        paths = self.pipe.get_processed_paths(chosen)
        assert len(post) == len(paths) == len(PICK)
        for k, i in enumerate(PICK):  # results in the order of the ticket list
            b = self.batch.get_processed_path(i)
            assert post[k].n_points == len(b["sampled"]) and post[k].smoothing_status == b["status"]
            same_processed(paths[k], b)
        return post, paths

    def close(self):
        self.pipe.close()
        self.batch.close()


def test_a_shuffled_subset_of_held_queries_equals_the_batch_planner_and_the_oracle():
    from pathplanning_amd._lib import PPError
    c = Case1()
    # the choice of queries was made with the oracle on the CPU: at least 4 of the 5 smooth with status >= 0 at this spacing
    h = O.Hybrid(c.w, O.params_array(), table=c.pipe.nonholo_table())
    sp = O.smoother_array(max_curvature=1.0 / O.DEFAULT_PARAMS["min_turning_radius"])
    want = []
    for i in PICK:
        r = h.search(c.starts[i], c.goals[i], int(c.seeds[i]))
        assert r["status"] == 0 and len(r["path_poses"]) >= 2
        want.append(O.postprocess(c.w, r, c.goals[i], O.params_array(), SPACING, sp))
    assert sum(x["status"] >= 0 for x in want) >= 4
    post, paths = c.check_subset()
    for k, x in enumerate(want):  # the tolerances of test_gpu_postprocess.run at 0.8 m
        g = paths[k]
        assert post[k].n_points == x["n_points"] and abs(post[k].length - x["length"]) < 1e-9
        assert np.array_equal(g["cusp"], x["cusp"]) and np.abs(g["sampled"] - x["resampled"]).max() < 1e-9
        assert post[k].smoothing_status == x["status"]
        if x["status"] >= 0:
            assert float(np.abs(g["smoothed"] - x["smoothed"]).max()) < 1e-5 and np.array_equal(g["path"], g["smoothed"])
        else:
            assert np.array_equal(g["path"], g["sampled"])
    # the 7 tickets that were not processed have no processed path
    for i in range(c.n):
        if i not in PICK:
            with pytest.raises(PPError) as e:
                c.pipe.get_processed_paths([c.tickets[i]])
            assert e.value.code == PP_ERR_INVALID and str(int(c.tickets[i])) in str(e.value)
    # ... nor has a processed ticket once it is released, by whatever route
    c.pipe.release([c.tickets[PICK[0]]])
    with pytest.raises(PPError):
        c.pipe.get_processed_paths([c.tickets[PICK[0]]])
    again = c.pipe.get_processed_paths([c.tickets[PICK[1]]], release=True)
    same_processed(again[0], paths[1])
    with pytest.raises(PPError):
        c.pipe.get_processed_paths([c.tickets[PICK[1]]])
    assert c.pipe.free_slots() == 16 - c.n + 2
    c.close()


def test_post_processing_beside_queries_in_flight_with_recycled_slots():
    """40 queries through 16 slots in dribbles: whatever is held is post-processed, fetched and released while the rest is being searched;
    every query equals the batch planner's post-processing bit for bit."""
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    ms.upload_nearest_cells(*O.world_nearest(w))
    rng = np.random.RandomState(42)
    n = 40
    starts, goals = valid_random_poses(rng, w, n), valid_random_poses(rng, w, n)
    seeds = np.arange(n, dtype=np.uint64) + 900
    for a in (starts, goals, seeds):  # the one long search of this stream (4067 expansions in the oracle) goes first: the others end beside it
        a[[0, 10]] = a[[10, 0]]
    pipe = pa.HybridAStarPipeline(val, capacity=16, max_nodes=32768, search_rows=8)
    pipe.initialize()
    batch = pa.HybridAStarBatch(val, max_batch=n, max_nodes=32768)
    batch.initialize(pipe.nonholo_table())
    ref = batch.search_batch(starts, goals, seeds)
    batch.postprocess(n, path_interpolation=SPACING)
    # submitted from device arrays: the host-array form frees its staging copies before it returns, which waits for the device -- and with it
    # for the searches this test wants to post-process beside
    import torch
    dev = torch.device("cuda", 0)
    d_starts, d_goals = torch.from_numpy(np.ascontiguousarray(starts)).to(dev), torch.from_numpy(np.ascontiguousarray(goals)).to(dev)
    d_seeds = torch.from_numpy(seeds.astype(np.int64)).to(dev)
    index_of, uses, nxt, done, beside, calls = {}, {}, 0, 0, 0, 0

    def check(tickets, res, post, paths):
        for k, t in enumerate(tickets):
            q = index_of[int(t)]
            assert res[k].status == ref[q].status and res[k].n_expanded == ref[q].n_expanded
            b = batch.get_processed_path(q)
            assert post[k].n_points == len(b["sampled"])
            same_processed(paths[k], b)

    def count_slots(tickets):
        for t in tickets:
            slot = pipe.lib.pp_pipeline_slot_of(pipe.h, C.c_uint64(int(t)))
            assert 0 <= slot < 16
            uses[slot] = uses.get(slot, 0) + 1

    # ---- by construction beside a query in flight: queries 1 .. 4 are held, then the long query 0 is submitted and not polled.  Two calls follow, the
    # second larger than the first, so the pipeline's buffers GROW with a query in flight.  Freeing device memory waits for the whole device --
    # here for the long search and then for the grid's idle waves, which stay about a second (PP_PIPE_IDLE_MS) while the host does not poll -- so a
    # call that frees takes more than a second; four plans' worth of descent (at most 2000 iterations of a few microseconds) takes milliseconds.
    # The bound sits between the two.
    first, took = pipe.submit_dev(d_starts, d_goals, d_seeds, n=4, offset=1)
    assert took == 4
    for i in range(4):
        index_of[first + i] = 1 + i
    got = drain(pipe, 4)
    held = sorted(got)
    res = [got[t] for t in held]
    count_slots(held)
    first, took = pipe.submit_dev(d_starts, d_goals, d_seeds, n=1, offset=0)
    assert took == 1 and pipe.in_flight() == 1
    index_of[first] = 0
    nxt = 5
    post = pipe.postprocess(held[:2], path_interpolation=SPACING)
    check(held[:2], res[:2], post, pipe.get_processed_paths(held[:2]))
    t1 = time.time()
    post = pipe.postprocess(held, path_interpolation=SPACING)  # 4 plans after 2: every buffer grows
    grow_s = time.time() - t1
    assert pipe.in_flight() == 1  # (nothing was polled: the long query is still the grid's)
    print("a post-processing call that grows its buffers beside a query in flight: %.1f ms" % (1e3 * grow_s))
    assert grow_s < 0.5
    check(held, res, post, pipe.get_processed_paths(held, release=True))
    beside, calls, done = 2, 2, 4

    # ---- the rest of the stream in dribbles: whatever is held is post-processed while the others are searched
    t0 = time.time()
    while done < n:
        if nxt < n and pipe.free_slots() > 0:
            first, took = pipe.submit_dev(d_starts, d_goals, d_seeds, n=min(n - nxt, 5), offset=nxt)
            for i in range(took):
                index_of[first + i] = nxt + i
            nxt += took
        tickets, res = pipe.poll(64, release=False)
        if len(tickets):
            count_slots(tickets)
            beside += pipe.in_flight() > 0
            calls += 1
            post = pipe.postprocess(tickets, path_interpolation=SPACING)
            check(tickets, res, post, pipe.get_processed_paths(tickets, release=True))
            done += len(tickets)
        assert time.time() - t0 < 120, "pipeline stalled"
    print("post-processing calls: %d, of them with queries in flight: %d; most uses of one slot: %d" % (calls, beside, max(uses.values())))
    assert beside >= 2 and max(uses.values()) >= 3  # (the two calls made by construction beside the long query, and whatever the dribbles add)
    assert pipe.in_flight() == 0 and pipe.free_slots() == 16
    pipe.close()
    batch.close()


def test_refusals_launch_nothing_and_leave_the_pipeline_usable():
    import pathplanning_amd as pa
    from pathplanning_amd._lib import PostResult, ptr
    c = Case1()
    lib, pipe = c.pipe.lib, c.pipe
    out = (PostResult * 32)()

    def refused(tickets, *words, n=None, max_points=2048, handle=None):
        t = np.ascontiguousarray(tickets, dtype=np.uint64)
        rc = lib.pp_pipeline_postprocess(handle or pipe.h, len(t) if n is None else n, ptr(t), C.c_float(SPACING), None, max_points, out)
        msg = lib.pp_last_error().decode()
        assert rc == PP_ERR_INVALID and all(wd in msg for wd in words), (rc, msg)

    held = [int(t) for t in c.tickets]
    # a long search (4067 expansions in the oracle) keeps its ticket in flight while it is named
    rng = np.random.RandomState(42)
    s40, g40 = valid_random_poses(rng, c.w, 40), valid_random_poses(rng, c.w, 40)
    flying = pipe.submit(s40[10:11], g40[10:11], np.array([910], dtype=np.uint64))
    assert len(flying) == 1
    refused([held[0], int(flying[0]), held[1]], "ticket %d" % int(flying[0]), "in flight")
    assert pipe.in_flight() == 1  # (it was refused while in flight, not after)
    drain(pipe, 1)
    pipe.release(flying)
    refused([held[0], int(flying[0])], "ticket %d" % int(flying[0]), "released")
    refused([held[0], 10 ** 9], "ticket %d" % 10 ** 9, "unknown")
    refused([held[3], held[4], held[3]], "ticket %d" % held[3], "twice")
    refused((held + held)[:17], "capacity")
    refused(held[:1], "capacity", n=-1)
    refused(held[:2], "max_points", max_points=7)
    refused(held[:2], "max_points", max_points=2049)
    t = np.ascontiguousarray(held[:2], dtype=np.uint64)
    assert lib.pp_pipeline_postprocess(pipe.h, 2, ptr(t), C.c_float(0.0), None, 2048, out) == PP_ERR_INVALID and b"path_interpolation" in lib.pp_last_error()
    assert lib.pp_pipeline_postprocess(pipe.h, 0, None, C.c_float(SPACING), None, 2048, out) == 0  # n == 0 is PP_OK
    # a map without nearest-cell grids
    w2, ms2, val2, _ = make_pair(256, 6, 4, ctx=c.ctx)
    bare = pa.HybridAStarPipeline(val2, capacity=16, max_nodes=32768, search_rows=8)
    bare.initialize(pipe.nonholo_table())
    rng = np.random.RandomState(5)
    bt = bare.submit(valid_random_poses(rng, w2, 2), valid_random_poses(rng, w2, 2), [1, 2])
    drain(bare, 2)
    refused(bt, "cell grids missing", handle=bare.h)
    bare.close()
    # after all that a valid call gives the subset's results
    c.check_subset()
    c.close()


def test_edge_statuses_failed_search_sample_limit_and_short_path():
    """One pipeline on an open 16 m box with a closed room in it: a goal inside the room (the search fails: n_points 0, status -1), a
    12 m plan that has more than max_points = 8 samples (-4, for that ticket only), a 5 m plan of 7 samples (smoothed as in the batch
    planner) and a 2.5 m plan of 4 samples (status 2, Smoother::Status::PathSize)."""
    import pathplanning_amd as pa
    lower, upper = (-8.0, -8.0, -np.pi), (8.0, 8.0, np.pi)
    w = O.World(lower=lower, upper=upper, resolution=0.1)
    for dx, dy, pose in ((4.3, 0.3, (4.0, 2.0, 0.0)), (4.3, 0.3, (4.0, 6.0, 0.0)), (0.3, 4.3, (2.0, 4.0, 0.0)), (0.3, 4.3, (6.0, 4.0, 0.0))):
        w.add_rectangle(dx, dy, pose)
    w.update()
    ctx = pa.Context(0)
    ms = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, 0.1)
    assert (ms.rows, ms.cols) == (w.rows, w.cols)
    ms.upload_dist2(w.d2())
    ms.upload_occupancy(w.occ())
    ms.upload_path_cost(w.pathcost())
    ms.upload_nearest_cells(*O.world_nearest(w))
    val = pa.StateValidatorOccupancyMap(ms)
    starts = np.array([(-5.0, -5.0, 0.0), (-6.0, -6.0, 0.3), (-5.0, 3.0, 0.0), (-5.0, 0.0, 0.0)])
    goals = np.array([(4.0, 4.0, 0.0), (-6.0, 5.5, 1.2), (0.0, 3.0, 0.0), (-2.5, 0.0, 0.0)])
    seeds = np.arange(4, dtype=np.uint64) + 50
    assert w.is_state_valid(np.vstack([starts, goals])).all()
    pipe = pa.HybridAStarPipeline(val, capacity=16, max_nodes=32768, search_rows=8)
    pipe.initialize()
    batch = pa.HybridAStarBatch(val, max_batch=4, max_nodes=32768)
    batch.initialize(pipe.nonholo_table())
    ref = batch.search_batch(starts, goals, seeds)
    assert [r.status for r in ref] == [-1, 0, 0, 0]
    tickets = pipe.submit(starts, goals, seeds)
    got = drain(pipe, 4)
    assert [got[int(t)].status for t in tickets] == [-1, 0, 0, 0]
    # the oracle's sample counts: 16, 7 and 4
    h = O.Hybrid(w, O.params_array(), table=pipe.nonholo_table())
    sp = O.smoother_array(max_curvature=1.0 / O.DEFAULT_PARAMS["min_turning_radius"])
    want = [None] + [O.postprocess(w, h.search(starts[q], goals[q], int(seeds[q])), goals[q], O.params_array(), SPACING, sp) for q in (1, 2, 3)]
    assert [x["n_points"] for x in want[1:]] == [16, 7, 4] and want[3]["status"] == 2
    for max_points in (2048, 8):
        bpost = batch.postprocess(4, path_interpolation=SPACING, max_points=max_points)
        order = [3, 1, 0, 2]
        post = pipe.postprocess([tickets[q] for q in order], path_interpolation=SPACING, max_points=max_points)
        paths = pipe.get_processed_paths([tickets[q] for q in order])
        for k, q in enumerate(order):
            assert (post[k].n_points, post[k].smoothing_status, post[k].iterations, post[k].length) == \
                (bpost[q].n_points, bpost[q].smoothing_status, bpost[q].iterations, bpost[q].length), (max_points, q)
            same_processed(paths[k], batch.get_processed_path(q))
        by_query = {q: post[k] for k, q in enumerate(order)}
        assert (by_query[0].n_points, by_query[0].smoothing_status) == (0, -1)
        assert (by_query[3].n_points, by_query[3].smoothing_status) == (4, 2)
        assert (by_query[2].n_points, by_query[2].smoothing_status) == (7, want[2]["status"]) and want[2]["status"] >= 0
        if max_points == 8:
            assert (by_query[1].n_points, by_query[1].smoothing_status) == (0, -4)
        else:
            assert (by_query[1].n_points, by_query[1].smoothing_status) == (16, want[1]["status"])
    pipe.close()
    batch.close()


def test_the_footprint_check_on_the_device_is_the_validators_verdict_on_the_smoothed_samples():
    """Plans searched with CAR3, held, post-processed four times under four footprints: the descent is untouched (sampled and smoothed
    paths equal the one-wave batch planner's, which smooths against the point validator), and the status is the batch planner's unless
    that is >= 0 and check_states with the footprint rejects a smoothed sample: then -2 and the sampled path."""
    import pathplanning_amd as pa
    w, ms, val, ctx = make_pair(256, 6, 3)
    ms.upload_nearest_cells(*O.world_nearest(w))
    g = R.Grid(w)
    rng = np.random.RandomState(8)
    n = 12
    starts, goals = R.valid_poses(rng, g, w, n, R.CAR3), R.valid_poses(rng, g, w, n, R.CAR3)
    seeds = np.arange(n, dtype=np.uint64) + 640
    car = pa.Footprint(ms, R.CAR3)
    footprints = [("none", None), ("point disc", pa.Footprint(ms, [(0.0, 0.0, val.min_safe_radius)])), ("CAR3", car), ("fat disc", pa.Footprint(ms, [(0.0, 0.0, 5.0)]))]
    pipe = pa.HybridAStarPipeline(val, capacity=16, max_nodes=32768, search_rows=8)
    pipe.initialize()
    pipe.set_footprint(car)
    batch = pa.HybridAStarBatch(val, max_batch=n, max_nodes=32768)  # one wave per query: the planner that takes a footprint
    batch.initialize(pipe.nonholo_table())
    batch.set_footprint(car)
    ref = batch.search_batch(starts, goals, seeds)
    batch.postprocess(n, path_interpolation=SPACING)
    want = [batch.get_processed_path(q) for q in range(n)]
    tickets = pipe.submit(starts, goals, seeds)
    got = drain(pipe, n)
    for q, t in enumerate(tickets):
        assert got[int(t)].status == ref[q].status and got[int(t)].n_expanded == ref[q].n_expanded
    kept = off = 0
    for name, fp in footprints:
        pipe.set_footprint(fp)  # legal: nothing is in flight, the slots are merely held
        post = pipe.postprocess(tickets, path_interpolation=SPACING)
        paths = pipe.get_processed_paths(tickets)
        for q in range(n):
            a, b = paths[q], want[q]
            assert post[q].n_points == len(b["sampled"])
            assert np.array_equal(a["sampled"], b["sampled"]) and np.array_equal(a["cusp"], b["cusp"]) and np.array_equal(a["smoothed"], b["smoothed"], equal_nan=True)
            expect = b["status"]
            if fp is not None and b["status"] >= 0 and len(b["smoothed"]) and not val.is_state_valid(b["smoothed"], footprint=fp).all():
                expect = -2
            assert a["status"] == expect and post[q].smoothing_status == expect, (name, q, a["status"], expect, b["status"])
            assert np.array_equal(a["path"], a["smoothed"] if expect >= 0 else a["sampled"], equal_nan=True)
            if name == "point disc":
                assert a["status"] != -2
            if name in ("CAR3", "fat disc") and len(b["sampled"]):
                kept += a["status"] >= 0
                off += a["status"] == -2
    print("under a real footprint: %d results kept their smoothed path, %d ended -2" % (kept, off))
    assert kept >= 1 and off >= 1
    pipe.close()
    batch.close()


def test_the_cpp_mirror_returns_what_hybrid_a_star_returns():
    """tests/cpp/test_pipeline_postprocess.cpp: GetPath(ticket) of Planner::HybridAStarPipeline against HybridAStar::SearchPath() + GetPath()"""
    from pathplanning_amd import build
    exe = build.build_pipeline_postprocess_test(verbose=False)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, env=dict(os.environ, PP_PIPE_ALLOW_SHARED_QUEUES="1"))
    print(r.stdout.decode())
    assert r.returncode == 0 and b"GetPath(ticket) == HybridAStar::GetPath() on every query" in r.stdout
