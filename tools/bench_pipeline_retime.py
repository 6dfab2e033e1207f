#!/usr/bin/env python3
"""What it costs to write decided waits into a fleet's timetables: the fleet of tools/bench_pipeline_deconflict.py -- ONE pipeline on the benchmark's
1024^2 synthetic map, --plans queries searched and HELD and given a speed profile, every plan paired with its --nearest nearest plans by start pose.
One pp_pipeline_deconflict_waits call with every vehicle barred from its start decides waits at stops; pa.planner.wait_holds turns them into holds.
Then, --reps times, in one process:
  speed profile: pa.HybridAStarPipeline.speed_profile without the rows coming down -- the call that puts fresh rows on the device before every retime
                 call below (a retime call accumulates), and the figure to compare with;
  library call:  pp_pipeline_retime into an array that exists (what a C or C++ caller pays), for the decided holds and for a synthetic list with one
                 hold at every plan's first inner stop;
  wrapper call:  pa.HybridAStarPipeline.retime, which returns one numpy record array, for the same two lists;
  rows down:     pa.HybridAStarPipeline.retime(rows=True) once per list: the rows a host route would have to move (there is no way to put rows back).
Host clock around each; median and spread of the repetitions.  There is no threshold: the call has no predecessor to compare with.

    python tools/bench_pipeline_retime.py [--plans 4096] [--nearest 32] [--horizon 60] [--dt 0.1] [--max-delay-steps 300] [--max-places 4] [--reps 7]
"""
import argparse
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
    ap.add_argument("--max-places", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_retime.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    from pathplanning_amd._lib import check, ptr
    from pathplanning_amd.planner import HOLD_DTYPE, RETIME_DTYPE, wait_holds
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
    pipe = pa.HybridAStarPipeline(val, pa.HybridAStarSearchParameters(), capacity=args.plans, max_nodes=args.max_nodes, search_rows=args.pipe_rows)
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
    lim = V.limits(spacing=float(np.float32(ms.resolution)), dwell=0.5)
    pairs = nearest_pairs(starts, args.nearest)
    t_start = np.round(np.random.RandomState(3).uniform(0.0, 0.5 * args.horizon, n), 3) + 0.0123
    kw = dict(t_from=0.0, t_to=args.horizon, dt=dt, margin=args.margin, hold_after=True)

    def fresh():
        t1 = time.perf_counter()
        recs = pipe.speed_profile(tickets, max_samples=args.max_samples, samples=False, **lim)
        return recs, 1e3 * (time.perf_counter() - t1)

    profiled, _ = fresh()
    t1 = time.perf_counter()
    waits = pipe.deconflict_waits(tickets, t_start, pairs=pairs, no_start_wait=np.ones(n, dtype=np.uint8), max_delay_steps=D, max_places=args.max_places, **kw)
    waits_ms = 1e3 * (time.perf_counter() - t1)
    decided, new_starts = wait_holds(waits, dt, t_start)
    assert np.array_equal(new_starts, t_start)  # (no vehicle may wait at its start)
    # the synthetic list: one hold at every plan's first inner stop (the timetable call lists the stops)
    plans, stops, _ = pipe.timetable(tickets, np.zeros((n, 0)), max_stops=8)
    first = []
    for i in range(n):
        inner = [int(st.row) for st in stops[i][:plans[i].n_listed] if 0 < st.row < plans[i].n_samples - 1]
        if inner:
            first.append((i, inner[0], 1.0))
    synthetic_holds = np.array(first, dtype=HOLD_DTYPE)
    c_tickets = np.ascontiguousarray(tickets, dtype=np.uint64)

    profile_ms, calls = [], []
    for name, holds in (("decided by deconflict_waits", decided), ("one hold at every plan's first inner stop", synthetic_holds)):
        timed = {"c_abi": [], "wrapper": []}
        out = np.zeros(n, dtype=RETIME_DTYPE)
        for rep in range(-1, args.reps):  # rep -1: warmed, untimed (the buffers are allocated there)
            for how in ("c_abi", "wrapper"):
                _, ms_profile = fresh()
                t1 = time.perf_counter()
                if how == "c_abi":
                    check(pipe.lib.pp_pipeline_retime(pipe.h, n, ptr(c_tickets), len(holds), ptr(holds) if len(holds) else None, None, ptr(out)))
                else:
                    wrapped = pipe.retime(tickets, holds)
                if rep >= 0:
                    timed[how].append(1e3 * (time.perf_counter() - t1))
                    profile_ms.append(ms_profile)
        assert wrapped.tobytes() == out.tobytes()
        fresh()
        t1 = time.perf_counter()
        _, rows = pipe.retime(tickets, holds, rows=True)
        rows_ms = 1e3 * (time.perf_counter() - t1)
        calls.append(dict(holds=name, n_holds=int(len(holds)), plans_with_a_hold=int((out["n_holds"] > 0).sum()), applied=int(((out["status"] == 0) & (out["n_holds"] > 0)).sum()),
                          not_a_stop=int((out["status"] == -2).sum()), negative_dwell=int((out["status"] == -3).sum()), without_a_profile=int((out["status"] == -1).sum()),
                          rows_rewritten=int(sum(p.n_samples - r["first_row"] for p, r in zip(plans, out) if r["status"] == 0 and r["first_row"] >= 0)),
                          seconds_held=float(out["held"].sum()), ms={k: stats(v) for k, v in timed.items()}, with_rows_down_ms=rows_ms,
                          bytes_down_with_rows=int(n * args.max_samples * 24 + n * RETIME_DTYPE.itemsize)))
    pipe.close()

    out = dict(tool="tools/bench_pipeline_retime.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=n, plans_found=int(found), nearest=args.nearest, pairs=int(len(pairs)), horizon=args.horizon, dt=dt, margin=args.margin, max_delay_steps=D,
               max_places=args.max_places, reps=args.reps, spacing=lim["spacing"], dwell=lim["dwell"], max_samples=args.max_samples, device=torch.cuda.get_device_name(0),
               samples=int(sum(r.n_samples for r in profiled if r.status == 0)), deconflict_waits_ms=waits_ms, waiting_at_a_stop=int(len(decided)),
               speed_profile_without_rows_ms=stats(profile_ms), retime=calls,
               not_measured=["the kernel's time apart from the call's", "more than one hold per plan at this scale", "the call beside queries in flight"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
