#!/usr/bin/env python3
"""What the space-time broad phase costs and what it buys, on the fleet of tools/bench_pipeline_deconflict.py: ONE pipeline on the benchmark's 1024^2
synthetic map, --plans queries searched and HELD and given a speed profile, a --horizon s horizon at dt = --dt, `hold_after`.  In one process:
  the list:      pp_pipeline_candidate_pairs at B in {16, 64, T} lattice times per box and D in {0, --max-delay-steps}: the size of the list and the
                 time of the call into arrays that exist (what a C or C++ caller pays) and through pa.HybridAStarPipeline.candidate_pairs, --reps times;
  host route:    ONCE, at B = 64 and the largest D: the poses down (conflicts(poses=True) over the extended horizon), the boxes and the all-pairs test in
                 numpy (tests/pair_restatement.py); its list is compared with the call's;
  the heuristic: pp_pipeline_conflicts over the D = 0 candidate list at B = 16; how many of the pairs it finds in conflict are absent from the
                 --nearest nearest list by start pose (tools/bench_pipeline_conflicts.py::nearest_pairs), which every earlier cost figure was measured on;
  the delays:    pp_pipeline_deconflict over the nearest list, and the pairs and levels of the largest-D candidate list at B = 16; with
                 --delay-over-candidates the call over that list too (levels, time, vehicles that wait).
Host clock around each; median and spread of the repetitions.  Nothing here is asserted against a threshold: the figures are recorded, and the
results so far are written after every section (`finished` says whether the run got to its end), so a section that runs long does not cost the others.

    python tools/bench_pipeline_candidate_pairs.py [--plans 4096] [--nearest 32] [--horizon 60] [--dt 0.1] [--max-delay-steps 300] [--reps 7] [--delay-reps 3]
                                                   [--out profiles/pipeline_candidate_pairs.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the pipeline runs although its streams may share hardware queues (the runtime's own number of queues is left as the environment has it)
os.environ.setdefault("PP_PIPE_ALLOW_SHARED_QUEUES", "1")


def stats(ms_list):
    return dict(median=float(np.median(ms_list)), min=float(min(ms_list)), max=float(max(ms_list)), runs=[float(x) for x in ms_list])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--plans", type=int, default=4096, help="held plans (= the pipeline's capacity)")
    ap.add_argument("--nearest", type=int, default=32)
    ap.add_argument("--horizon", type=float, default=60.0)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--margin", type=float, default=0.5)
    ap.add_argument("--max-delay-steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--delay-reps", type=int, default=3, help="repetitions of each of the two delay calls")
    ap.add_argument("--delay-over-candidates", action="store_true",
                    help="also run the delay call over the largest-D candidate list; on the default fleet that list is 3.8 M pairs in 2271 levels and the call did not finish in 7 minutes")
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_candidate_pairs.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    from pathplanning_amd._lib import ConflictParams, ConflictResult, DelayParams, PairParams, PairSummary, TrajectoryResult, check, ptr
    from pathplanning_amd.planner import DELAY_DTYPE, conflict_lattice, delay_levels
    import pair_restatement as PR
    import speed_restatement as V
    from bench_pipeline_conflicts import nearest_pairs
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = pa.Context(0)
    m, _ = synthetic.make_map_product(ctx, args.cells, args.obstacles, seed=1, reference_order=False)
    ms, val = synthetic.upload(ctx, m)
    ms.update_gvd()
    reach = synthetic.reachable_mask(val, m)
    starts = synthetic.sample_valid_poses(val, m, args.plans, seed=1000, reachable=reach)
    goals = synthetic.sample_valid_poses(val, m, args.plans, seed=2000, reachable=reach)
    params = pa.HybridAStarSearchParameters()
    pipe = pa.HybridAStarPipeline(val, params, capacity=args.plans, max_nodes=args.max_nodes, search_rows=args.pipe_rows)
    pipe.initialize()
    tickets = pipe.submit(starts, goals, np.arange(args.plans, dtype=np.uint64))
    assert len(tickets) == args.plans
    t0 = time.perf_counter()
    done = found = 0
    while done < args.plans:
        got, res = pipe.poll(4096, release=False)
        found += sum(r.status == 0 for r in res[:len(got)])
        done += len(got)
        if time.perf_counter() - t0 > 600:
            raise RuntimeError("pipeline stalled: %d of %d results" % (done, args.plans))

    n, D, dt = args.plans, args.max_delay_steps, args.dt
    every = n * (n - 1) // 2
    lim = V.limits(spacing=float(np.float32(ms.resolution)))
    near = nearest_pairs(starts, args.nearest)
    t_start = np.round(np.random.RandomState(3).uniform(0.0, 0.5 * args.horizon, n), 3) + 0.0123
    kw = dict(t_from=0.0, t_to=args.horizon, dt=dt, margin=args.margin, hold_after=True)
    k0, T = conflict_lattice(kw["t_from"], kw["t_to"], dt)
    pipe.speed_profile(tickets, max_samples=args.max_samples, samples=False, **lim)
    print("fleet ready: %d plans, %d found, T = %d" % (n, found, T), flush=True)

    c_tickets, c_starts = np.ascontiguousarray(tickets, dtype=np.uint64), np.ascontiguousarray(t_start, dtype=np.float64)
    lattice = ConflictParams(kw["t_from"], kw["t_to"], dt, args.margin, 0, 1)
    out = dict(tool="tools/bench_pipeline_candidate_pairs.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=n, plans_found=int(found), every_pair=every, lattice_times=T, horizon=args.horizon, dt=dt, margin=args.margin, hold_after=True, reps=args.reps,
               delay_reps=args.delay_reps, spacing=lim["spacing"], device=torch.cuda.get_device_name(0), finished=False)

    def save(**more):
        """the results so far: a section that runs long must not cost the ones before it"""
        out.update(more)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    # ---- the list: size and time, through the C ABI and through the wrapper
    lists, table = {}, []
    for d in sorted({0, D}):
        for B in sorted({16, 64, T}):
            wrapped = pipe.candidate_pairs(tickets, t_start, times_per_box=B, max_delay_steps=d, **kw)  # (untimed: the buffers are allocated here, and it sizes the arrays)
            count = int(wrapped[2].n_found)
            c_pairs, c_first, c_sum = np.zeros((max(count, 1), 2), dtype=np.int32), np.zeros(max(count, 1), dtype=np.int32), PairSummary()
            c_params = PairParams(DelayParams(lattice, d, 0), B, count)
            timed = {"c_abi": [], "wrapper": []}
            for rep in range(args.reps):
                t1 = time.perf_counter()
                check(pipe.lib.pp_pipeline_candidate_pairs(pipe.h, n, ptr(c_tickets), ptr(c_starts), C.byref(c_params), ptr(c_pairs), ptr(c_first), None, C.byref(c_sum)))
                timed["c_abi"].append(1e3 * (time.perf_counter() - t1))
                t1 = time.perf_counter()
                wrapped = pipe.candidate_pairs(tickets, t_start, times_per_box=B, max_delay_steps=d, **kw)
                timed["wrapper"].append(1e3 * (time.perf_counter() - t1))
            same = bool(c_sum.n_found == count and wrapped[0].tobytes() == c_pairs[:count].tobytes() and wrapped[1].tobytes() == c_first[:count].tobytes())
            lists[(d, B)] = wrapped[0].copy()
            table.append(dict(max_delay_steps=d, times_per_box=B, boxes_per_plan=int(c_sum.n_boxes), plans_boxed=int(c_sum.n_boxed), reach=float(c_sum.reach), pairs=count,
                              share_of_every_pair=count / every, c_abi_equals_wrapper=same, candidate_pairs_ms={k: stats(v) for k, v in timed.items()}))
            print("D = %d, B = %d: %d pairs (%.2f %% of every pair), %.2f ms through the C ABI, %.2f ms through the wrapper" % (
                d, B, count, 100.0 * count / every, np.median(timed["c_abi"]), np.median(timed["wrapper"])), flush=True)
            save(lists=table)

    # ---- the host route, once: poses down, boxes and the all-pairs test in numpy
    t1 = time.perf_counter()
    wider = dict(kw, t_from=(k0 - D - 0.5) * dt)
    poses = np.array(pipe.conflicts(tickets, t_start, pairs=[(0, 1)], poses=True, **wider)[2], dtype=np.float64)
    t2 = time.perf_counter()
    host = PR.candidate_pairs(poses, T, D, 64, [(0.0, 0.0, float(val.min_safe_radius))], args.margin)
    t3 = time.perf_counter()
    host_route = dict(times_per_box=64, max_delay_steps=D, ms=1e3 * (t3 - t1), poses_ms=1e3 * (t2 - t1), pairs=int(host["n_found"]),
                      equals_the_calls_list=bool(np.array_equal(host["pairs"], lists[(D, 64)])))
    del poses
    save(host_route=host_route)
    print("host route: %.0f ms (%.0f ms of it the poses), %d pairs, equal to the call's list: %s" % (host_route["ms"], host_route["poses_ms"], host_route["pairs"],
                                                                                                host_route["equals_the_calls_list"]), flush=True)

    # ---- what the nearest list has been missing: the conflict call over the D = 0 candidate list
    cand0 = np.ascontiguousarray(lists[(0, 16)])
    plan_recs, pair_recs = (TrajectoryResult * n)(), (ConflictResult * max(len(cand0), 1))()
    timed = []
    for rep in range(args.reps):
        t1 = time.perf_counter()
        check(pipe.lib.pp_pipeline_conflicts(pipe.h, n, ptr(c_tickets), ptr(c_starts), len(cand0), ptr(cand0), C.byref(lattice), None, plan_recs, pair_recs))
        timed.append(1e3 * (time.perf_counter() - t1))
    status = np.frombuffer(pair_recs, dtype=np.dtype(ConflictResult))["status"][:len(cand0)]
    in_conflict = cand0[status == 1]
    key = lambda p: np.minimum(p[:, 0], p[:, 1]).astype(np.int64) * n + np.maximum(p[:, 0], p[:, 1])
    missed = int((~np.isin(key(in_conflict), key(near))).sum())
    heuristic = dict(nearest=args.nearest, nearest_pairs=int(len(near)), candidate_pairs=int(len(cand0)), nearest_pairs_among_the_candidates=int(np.isin(key(near), key(cand0)).sum()),
                     pairs_in_conflict_over_the_candidates=int(len(in_conflict)), of_them_absent_from_the_nearest_list=missed, conflicts_ms=stats(timed))
    print("conflicts over %d candidates: %d pairs in conflict, %d of them absent from the %d-nearest list (%d pairs); %.2f ms" % (
        len(cand0), len(in_conflict), missed, args.nearest, len(near), np.median(timed)), flush=True)
    save(heuristic=heuristic)

    # ---- the delays: over the candidate list against the nearest list
    c_params = DelayParams(lattice, D, 0)
    delays = {}
    for name, pairs in (("nearest", np.ascontiguousarray(near, dtype=np.int32)), ("candidates", np.ascontiguousarray(lists[(D, 16)]))):
        level = delay_levels(n, pairs)
        delays[name] = dict(pairs=int(len(pairs)), levels=int(level.max()) + 1, largest_level=int(np.bincount(level).max()))
        save(deconflict=delays)
        print("deconflict over %s: %d pairs in %d levels ..." % (name, len(pairs), delays[name]["levels"]), flush=True)
        if name == "candidates" and not args.delay_over_candidates:
            delays[name]["deconflict_ms"] = None  # (levels and pairs are recorded; the call is run on request)
            continue
        c_out = np.zeros(n, dtype=DELAY_DTYPE)
        timed = []
        for rep in range(-1, args.delay_reps):  # rep -1: warmed, untimed
            t1 = time.perf_counter()
            check(pipe.lib.pp_pipeline_deconflict(pipe.h, n, ptr(c_tickets), ptr(c_starts), len(pairs), ptr(pairs), C.byref(c_params), ptr(c_out)))
            if rep >= 0:
                timed.append(1e3 * (time.perf_counter() - t1))
        delays[name].update(scheduled=int((c_out["status"] == 0).sum()),
                            waiting=int((c_out["delay_steps"] > 0).sum()), without_a_clear_delay=int((c_out["status"] == 1).sum()), without_a_plan=int((c_out["status"] == -1).sum()),
                            longest_delay_steps=int(c_out["delay_steps"].max()), candidates_tried=int(c_out["n_tried"].sum()), deconflict_ms=stats(timed))
        print("deconflict over %s: %d pairs, %d levels, %d wait, %d without a clear delay, %.1f ms" % (name, len(pairs), delays[name]["levels"], delays[name]["waiting"],
                                                                                                  delays[name]["without_a_clear_delay"], np.median(timed)), flush=True)
        save(deconflict=delays)
    pipe.close()
    save(finished=True, not_measured=["each kernel's time apart from the call's", "a multi-disc footprint at this scale", "the host route more than once, or at another B",
                                      "deconflict_tracks over the list", "the conflict call over every pair of the fleet"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
