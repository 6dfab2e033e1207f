#!/usr/bin/env python3
"""What it costs to ask a fleet's held plans who meets whom, and when: ONE pipeline on the benchmark's 1024^2 synthetic map, --plans queries searched
and HELD and given a speed profile, every plan paired with its --nearest nearest plans by start pose, a --horizon s horizon at dt = --dt, then, in
the same process, two routes to the same pair records:
  device route: one pp_pipeline_conflicts call over every held ticket (k_trajectory_tickets, one wave per plan; k_conflict_pairs, one wave per
                pair) -- through the Python wrapper without and with the poses copied back, and the library call alone into arrays that exist
                (the wrapper also builds one Python object per record), --reps times each;
  host route:   what a caller could do before that call existed -- speed_profile WITH its rows (a copy of n x max_samples x 24 B), get_path_of per
                ticket, the edges rebuilt on the host (as tools/bench_pipeline_speed_profile.py rebuilds them), the rule of include/pp_hip.h evaluated
                in numpy (tests/conflict_restatement.py, the comparator of the GPU test) -- --host-reps times.
Host clock around each route; median of the repetitions and their spread.  The two routes' records are compared under the rule of
tests/test_gpu_pipeline_conflicts.py: plan records and n_times equal, min_separation within 1e-9, status / n_conflict / t_first equal on pairs with no
undecided time, t_min equal where the minimum is decided.

    python tools/bench_pipeline_conflicts.py [--plans 4096] [--nearest 32] [--horizon 60] [--dt 0.1] [--reps 7] [--host-reps 3] [--out profiles/pipeline_conflicts.json]
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


def nearest_pairs(starts, k):
    """every plan with its k nearest by start position, each pair once, as (i, j) with i < j"""
    xy = np.asarray(starts)[:, :2]
    pairs = set()
    for i in range(len(xy)):
        d = np.hypot(*(xy - xy[i]).T)
        d[i] = np.inf
        for j in np.argsort(d, kind="stable")[:k]:
            pairs.add((min(i, int(j)), max(i, int(j))))
    return np.array(sorted(pairs), dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--plans", type=int, default=4096, help="held plans (= the pipeline's capacity)")
    ap.add_argument("--nearest", type=int, default=32)
    ap.add_argument("--horizon", type=float, default=60.0)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--margin", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_conflicts.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    from pathplanning_amd._lib import ConflictParams, ConflictResult, TrajectoryResult, check, ptr
    import conflict_restatement as CR
    import locate_restatement as R
    import speed_restatement as V
    from bench_pipeline_speed_profile import host_plan
    from test_gpu_pipeline_stamp import RS_FEED
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
    index_of = {int(t): i for i, t in enumerate(tickets)}
    status = [None] * args.plans
    t0 = time.perf_counter()
    done = 0
    while done < args.plans:
        got, res = pipe.poll(4096, release=False)
        for k, t in enumerate(got):
            status[index_of[int(t)]] = res[k].status
        done += len(got)
        if time.perf_counter() - t0 > 600:
            raise RuntimeError("pipeline stalled: %d of %d results" % (done, args.plans))

    rs = pa.ReedsSheppPaths(ctx, params.min_turning_radius, params.direction_switching_cost, params.reverse_cost_multiplier, params.forward_cost_multiplier)
    prims = params.primitives()
    lim = V.limits(spacing=float(np.float32(ms.resolution)))
    discs = [(0.0, 0.0, float(np.float32(val.min_safe_radius)))]
    pairs = nearest_pairs(starts, args.nearest)
    t_start = np.round(np.random.RandomState(3).uniform(0.0, 0.5 * args.horizon, args.plans), 3) + 0.0123
    kw = dict(t_from=0.0, t_to=args.horizon, dt=args.dt, margin=args.margin, hold_after=True)

    timed = {"records_only": [], "with_poses": [], "c_abi_records_only": []}
    device = None
    c_tickets, c_starts = np.ascontiguousarray(tickets, dtype=np.uint64), np.ascontiguousarray(t_start, dtype=np.float64)
    c_params = ConflictParams(kw["t_from"], kw["t_to"], kw["dt"], kw["margin"], 0, 1)
    c_plans, c_out = (TrajectoryResult * args.plans)(), (ConflictResult * len(pairs))()
    for rep in range(-1, args.reps):  # rep -1: warmed, untimed (the buffers are allocated there)
        pipe.speed_profile(tickets, max_samples=args.max_samples, samples=False, **lim)
        # the library call alone, into arrays that exist: what a C or C++ caller pays (the Python wrapper below also builds a list of record objects)
        t1 = time.perf_counter()
        check(pipe.lib.pp_pipeline_conflicts(pipe.h, args.plans, ptr(c_tickets), ptr(c_starts), len(pairs), ptr(pairs), C.byref(c_params), None, c_plans, c_out))
        if rep >= 0:
            timed["c_abi_records_only"].append(1e3 * (time.perf_counter() - t1))
        for name, poses in (("records_only", False), ("with_poses", True)):
            t1 = time.perf_counter()
            got = pipe.conflicts(tickets, t_start, pairs=pairs, poses=poses, **kw)
            if rep >= 0:
                timed[name].append(1e3 * (time.perf_counter() - t1))
            device = got if not poses else device
    host_ms, host = [], None
    for rep in range(args.host_reps):
        t1 = time.perf_counter()
        recs, rows = pipe.speed_profile(tickets, max_samples=args.max_samples, **lim)
        plans = [host_plan(R, RS_FEED, pipe, rs, prims, t, status[q], goals[q]) for q, t in enumerate(tickets)]
        host = CR.conflicts(plans, [r if len(r) else None for r in rows], t_start, [tuple(p) for p in pairs], discs, lim["a_acc"], lim["a_dec"], **kw)
        host_ms.append(1e3 * (time.perf_counter() - t1))
    pipe.close()

    tau, traj, want = host
    wrong_plans = sum((a.status, a.n_present, a.first, a.last, a.s_enter, a.s_leave) != (b["status"], b["n_present"], b["first"], b["last"], b["s_enter"], b["s_leave"])
                      for a, b in zip(device[0], traj))
    times = undecided = wrong = conflicts = 0
    for a, b in zip(device[1], want):
        if a.n_times != b["n_times"] or (b["status"] in (-1, 2) and a.status != b["status"]):
            wrong += 1
            continue
        if b["status"] in (-1, 2):
            continue
        sep = b["separation"]
        rest = sep[sep.view(np.uint64) != np.float64(sep.min()).view(np.uint64)]
        min_decided = not len(rest) or rest.min() > sep.min() + CR.EPS
        times += b["n_times"]
        undecided += b["undecided"] + (0 if min_decided else 1)
        ok = abs(a.min_separation - b["min_separation"]) <= 1e-9 and (not min_decided or a.t_min == b["t_min"])
        if b["undecided"] == 0:
            ok = ok and (a.status, a.n_conflict, a.t_first) == (b["status"], b["n_conflict"], b["t_first"])
        wrong += not ok
        conflicts += a.status == 1
    agreement = dict(plans=len(traj), plan_records_that_disagree=int(wrong_plans), pairs=len(want), pairs_in_conflict=int(conflicts), pair_times=int(times),
                     undecided_pair_times=int(undecided), pair_records_that_disagree=int(wrong))

    out = dict(tool="tools/bench_pipeline_conflicts.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=args.plans, plans_found=sum(s == 0 for s in status), nearest=args.nearest, pairs=int(len(pairs)), lattice_times=len(tau), horizon=args.horizon, dt=args.dt,
               margin=args.margin, hold_after=True, reps=args.reps, host_reps=args.host_reps, spacing=lim["spacing"], max_samples=args.max_samples, discs=discs,
               device=torch.cuda.get_device_name(0), agreement=agreement, conflicts_ms={k: stats(v) for k, v in timed.items()}, host_route_ms=stats(host_ms),
               ratio_host_route_over_conflicts=float(np.median(host_ms) / np.median(timed["records_only"])),
               ratio_host_route_over_c_abi=float(np.median(host_ms) / np.median(timed["c_abi_records_only"])),
               not_measured=["the two kernels' time apart from the call's", "a multi-disc footprint at this scale", "every pair of the fleet (n (n - 1) / 2 = 8.4 M pairs)"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert agreement["plan_records_that_disagree"] == 0 and agreement["pair_records_that_disagree"] == 0, "the two routes disagree: %r" % agreement


if __name__ == "__main__":
    main()
