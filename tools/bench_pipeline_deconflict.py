#!/usr/bin/env python3
"""What it costs to give a fleet's held plans start delays that clear their conflicts: ONE pipeline on the benchmark's 1024^2 synthetic map, --plans
queries searched and HELD and given a speed profile, every plan paired with its --nearest nearest plans by start pose (the pair list of
tools/bench_pipeline_conflicts.py), a --horizon s horizon at dt = --dt, delays of up to --max-delay-steps lattice steps, priority = the index of a
plan.  Then, in the same process, three routes to the delays:
  library call:  pp_pipeline_deconflict into an array that exists (what a C or C++ caller pays) -- the levels and partner lists on the host, the
                 extended trajectory (k_trajectory_tickets), one k_delay_level launch per level -- --reps times;
  wrapper call:  pa.HybridAStarPipeline.deconflict, which returns one numpy record array, --reps times;
  host loop:     what a caller could do before the call existed -- level by level, pp_pipeline_conflicts (the C ABI, records into arrays that exist, the
                 pairs of the level's undecided vehicles with their scheduled partners) over ALL tickets, every vehicle with a conflict waits one more
                 step, and again until the level is clear or out of delays -- once, and given up after --host-budget seconds.
Host clock around each; median and spread of the repetitions.  The host loop forms u = tau - t_start' afresh, so its delays agree with the call's to
rounding; the vehicles whose delay differs are counted, not asserted.

    python tools/bench_pipeline_deconflict.py [--plans 4096] [--nearest 32] [--horizon 60] [--dt 0.1] [--max-delay-steps 300] [--reps 7] [--out profiles/pipeline_deconflict.json]
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
    ap.add_argument("--host-budget", type=float, default=150.0, help="seconds after which the host loop is given up")
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_deconflict.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    from pathplanning_amd._lib import ConflictParams, ConflictResult, DelayParams, TrajectoryResult, check, ptr
    from pathplanning_amd.planner import DELAY_DTYPE, delay_levels
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
    lim = V.limits(spacing=float(np.float32(ms.resolution)))
    pairs = nearest_pairs(starts, args.nearest)
    t_start = np.round(np.random.RandomState(3).uniform(0.0, 0.5 * args.horizon, n), 3) + 0.0123
    kw = dict(t_from=0.0, t_to=args.horizon, dt=dt, margin=args.margin, hold_after=True)
    level = delay_levels(n, pairs)
    n_levels = int(level.max()) + 1
    pipe.speed_profile(tickets, max_samples=args.max_samples, samples=False, **lim)

    c_tickets, c_starts = np.ascontiguousarray(tickets, dtype=np.uint64), np.ascontiguousarray(t_start, dtype=np.float64)
    lattice = ConflictParams(kw["t_from"], kw["t_to"], dt, args.margin, 0, 1)
    c_params = DelayParams(lattice, D, 0)
    c_out = np.zeros(n, dtype=DELAY_DTYPE)
    timed = {"c_abi": [], "wrapper": []}
    wrapped = None
    for rep in range(-1, args.reps):  # rep -1: warmed, untimed (the buffers are allocated there)
        t1 = time.perf_counter()
        check(pipe.lib.pp_pipeline_deconflict(pipe.h, n, ptr(c_tickets), ptr(c_starts), len(pairs), ptr(pairs), C.byref(c_params), ptr(c_out)))
        if rep >= 0:
            timed["c_abi"].append(1e3 * (time.perf_counter() - t1))
        t1 = time.perf_counter()
        wrapped = pipe.deconflict(tickets, t_start, pairs=pairs, max_delay_steps=D, **kw)
        if rep >= 0:
            timed["wrapper"].append(1e3 * (time.perf_counter() - t1))
    assert wrapped.tobytes() == c_out.tobytes()
    device = c_out.copy()

    # ---- the host loop over pp_pipeline_conflicts
    below = [[] for _ in range(n)]
    for a, b in pairs.tolist():
        below[max(a, b)].append(min(a, b))
    plan_recs, pair_recs = (TrajectoryResult * n)(), (ConflictResult * len(pairs))()
    pair_status = np.frombuffer(pair_recs, dtype=np.dtype(ConflictResult))["status"]
    plan_status = np.frombuffer(plan_recs, dtype=np.dtype(TrajectoryResult))["status"]
    delay = np.full(n, -2, dtype=np.int64)  # -2: not decided yet; -1: no clear delay, or no plan
    now = c_starts.copy()
    calls = 0
    t1 = time.perf_counter()
    finished = True
    for l in range(n_levels):
        active = {int(i): 0 for i in np.flatnonzero(level == l)}
        while active:
            listed = np.array([(j, i) for i in active for j in below[i] if delay[j] >= 0], dtype=np.int32).reshape(-1, 2)
            some = listed if len(listed) else np.zeros((1, 2), dtype=np.int32)  # (a list that exists: NULL would mean every pair)
            check(pipe.lib.pp_pipeline_conflicts(pipe.h, n, ptr(c_tickets), ptr(now), len(listed), ptr(some), C.byref(lattice), None, plan_recs, pair_recs))
            calls += 1
            hit = set(listed[pair_status[:len(listed)] == 1, 1].tolist()) if len(listed) else set()
            for i in list(active):
                if plan_status[i] < 0:
                    delay[i] = -1
                    del active[i]
                elif i not in hit:
                    delay[i] = active.pop(i)
                elif active[i] == D:
                    delay[i] = -1
                    now[i] = c_starts[i]
                    del active[i]
                else:
                    active[i] += 1
                    now[i] = c_starts[i] + float(active[i]) * dt
            if time.perf_counter() - t1 > args.host_budget:
                finished = False
                break
        if not finished:
            break
    host_ms = 1e3 * (time.perf_counter() - t1)
    pipe.close()

    decided = delay > -2
    differ = int((delay[decided] != device["delay_steps"][decided]).sum())
    out = dict(tool="tools/bench_pipeline_deconflict.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=n, plans_found=int(found), nearest=args.nearest, pairs=int(len(pairs)), levels=n_levels, largest_level=int(np.bincount(level).max()),
               lattice_times=int(round(args.horizon / dt)) + 1, horizon=args.horizon, dt=dt, margin=args.margin, hold_after=True, max_delay_steps=D, reps=args.reps,
               spacing=lim["spacing"], device=torch.cuda.get_device_name(0),
               scheduled=int((device["status"] == 0).sum()), waiting=int((device["delay_steps"] > 0).sum()), without_a_clear_delay=int((device["status"] == 1).sum()),
               without_a_plan=int((device["status"] == -1).sum()), longest_delay_steps=int(device["delay_steps"].max()), candidates_tried=int(device["n_tried"].sum()),
               deconflict_ms={k: stats(v) for k, v in timed.items()},
               host_loop=dict(ms=host_ms, conflicts_calls=calls, finished=finished, vehicles_decided=int(decided.sum()), delays_that_differ_from_the_calls=differ),
               ratio_host_loop_over_c_abi=float(host_ms / np.median(timed["c_abi"])) if finished else None,
               not_measured=["k_delay_level's time apart from the call's", "a multi-disc footprint at this scale", "every pair of the fleet (n launches of one wave)",
                             "the host loop repeated (it runs once)"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
