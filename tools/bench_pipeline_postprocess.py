#!/usr/bin/env python3
"""What sampled and smoothed paths cost the streaming pipeline (pp_pipeline_postprocess): ONE pipeline on the benchmark's 1024^2 synthetic
map, the same query stream twice per repetition --
  release:      polling with release (the search stage alone, as bench.py drives it without paths);
  postprocess:  completions are HELD, post-processed in windows of --window tickets at --spacing metres while the rest of the stream is
                being searched (k_postprocess_tickets on the control stream, beside the persistent search grid), then released.
Host clock from the first submission to the last poll; median of --reps windows and their spread; milliseconds per post-processing call.
The label grids the smoother reads are built on the device from the map's occupancy (pp_map_update_gvd, exact transform).

    python tools/bench_pipeline_postprocess.py [--queries 32768] [--reps 5] [--out profiles/pipeline_postprocess.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the pipeline runs although its streams may share hardware queues (the runtime's own number of queues is left as the environment has it)
os.environ.setdefault("PP_PIPE_ALLOW_SHARED_QUEUES", "1")


def stream(pipe, d_starts, d_goals, d_seeds, n, chunk, post=None, stall_s=600.0):
    """n queries through the pipeline, submissions of `chunk` as slots come free.  post = None: polled with release; post = (window,
    spacing): held, post-processed `window` tickets at a time, released.  -> (seconds, plans found, post-processing call times [s],
    smoothing statuses seen)"""
    nxt = done = solved = 0
    held = np.empty(0, dtype=np.uint64)
    calls, statuses = [], {}
    t0 = time.perf_counter()

    def process(tickets):
        t1 = time.perf_counter()
        res = pipe.postprocess(tickets, path_interpolation=post[1])
        calls.append(time.perf_counter() - t1)
        for r in res:
            statuses[r.smoothing_status] = statuses.get(r.smoothing_status, 0) + 1
        pipe.release(tickets)

    while done < n:
        k = min(chunk, n - nxt)
        if k > 0 and pipe.free_slots() >= k:
            _, took = pipe.submit_dev(d_starts, d_goals, d_seeds, n=k, offset=nxt)
            nxt += took
        tickets, res = pipe.poll_array(4096) if post is None else pipe.poll_array_held(4096)
        if len(tickets):
            done += len(tickets)
            solved += int((res["status"] == 0).sum())
            if post is not None:
                held = np.concatenate([held, tickets])
                while len(held) >= post[0] or (done == n and len(held)):
                    process(held[:post[0]])
                    held = held[post[0]:]
        if time.perf_counter() - t0 > stall_s:
            raise RuntimeError("pipeline stalled: %d of %d results after %.0f s" % (done, n, stall_s))
    return time.perf_counter() - t0, solved, calls, statuses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--queries", type=int, default=32768, help="queries per timed window (at least a second of work)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=8192)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--window", type=int, default=256, help="tickets per post-processing call")
    ap.add_argument("--spacing", type=float, default=0.8, help="path interpolation [m]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_postprocess.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    ctx = pa.Context(0)
    m, _ = synthetic.make_map_product(ctx, args.cells, args.obstacles, seed=1, reference_order=False)
    ms, val = synthetic.upload(ctx, m)
    ms.update_gvd()  # the nearest-obstacle / nearest-edge cell grids (and the distance / path-cost grids they belong to)
    reach = synthetic.reachable_mask(val, m)
    starts = synthetic.sample_valid_poses(val, m, args.queries, seed=1000, reachable=reach)
    goals = synthetic.sample_valid_poses(val, m, args.queries, seed=2000, reachable=reach)
    d_starts, d_goals = torch.from_numpy(np.ascontiguousarray(starts)).to(dev), torch.from_numpy(np.ascontiguousarray(goals)).to(dev)
    d_seeds = torch.arange(args.queries, dtype=torch.int64, device=dev)

    pipe = pa.HybridAStarPipeline(val, pa.HybridAStarSearchParameters(), capacity=args.capacity, max_nodes=args.max_nodes, search_rows=args.pipe_rows)
    pipe.initialize()
    modes = {"release": None, "postprocess": (args.window, args.spacing)}
    rates = {name: [] for name in modes}
    call_ms, statuses, found = [], {}, {}
    for rep in range(-1, args.reps):  # rep -1: both modes warmed, untimed
        for name, post in modes.items():
            dt, solved, calls, st = stream(pipe, d_starts, d_goals, d_seeds, args.queries, args.chunk, post)
            found[name] = solved
            if rep >= 0:
                rates[name].append(args.queries / dt)
                call_ms += [1e3 * c for c in calls]
                for k, v in st.items():
                    statuses[str(k)] = statuses.get(str(k), 0) + v
    pipe.close()

    out = dict(tool="tools/bench_pipeline_postprocess.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               queries_per_window=args.queries, reps=args.reps, capacity=args.capacity, submit_chunk=args.chunk, search_rows=pipe.search_rows,
               tickets_per_postprocess_call=args.window, path_interpolation=args.spacing, device=torch.cuda.get_device_name(0), modes={})
    for name, r in rates.items():
        out["modes"][name] = dict(plans_per_s_median=float(np.median(r)), plans_per_s_min=float(min(r)), plans_per_s_max=float(max(r)), plans_per_s_runs=[float(x) for x in r],
                                  plans_found=found[name])
    out["postprocess_call_ms"] = dict(median=float(np.median(call_ms)), min=float(min(call_ms)), max=float(max(call_ms)), calls=len(call_ms))
    out["smoothing_statuses"] = statuses
    out["ratio_release_over_postprocess"] = out["modes"]["release"]["plans_per_s_median"] / out["modes"]["postprocess"]["plans_per_s_median"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
