#!/usr/bin/env python3
"""What a timetable look-up costs and what it replaces, on the fleet of tools/bench_pipeline_deconflict.py: ONE pipeline on the benchmark's 1024^2
synthetic map, --plans queries searched and HELD and given a speed profile whose rows stay on the device.  In one process:
  the call:      pp_pipeline_timetable with ONE look-up per plan by arc length (a located vehicle's set-point, its time on the timetable and its next
                 stop) and with EIGHT per plan by time, 16 stops listed per plan: the time of the call into arrays that exist (what a C or C++ caller
                 pays) and through pa.HybridAStarPipeline.timetable, --reps times;
  host route:    what a caller did without the call, --host-reps times: pp_pipeline_speed_profile with the rows downloaded, then the restatement's
                 arithmetic in numpy (tests/timetable_restatement.py: row search, step, stops, next stop; no pose); its s, t, v and stops are compared
                 with the call's, bit for bit.
Host clock around each; median and spread of the repetitions.  Nothing here is asserted against a threshold: the figures are recorded.

    python tools/bench_pipeline_timetable.py [--plans 4096] [--reps 21] [--host-reps 3] [--out profiles/pipeline_timetable.json]
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

# the pipeline runs although its streams may share hardware queues (the runtime's own number of queues is left as the environment has it)
os.environ.setdefault("PP_PIPE_ALLOW_SHARED_QUEUES", "1")


def stats(ms_list):
    return dict(median=float(np.median(ms_list)), min=float(min(ms_list)), max=float(max(ms_list)), runs=[float(x) for x in ms_list])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--plans", type=int, default=4096, help="held plans (= the pipeline's capacity)")
    ap.add_argument("--max-stops", type=int, default=16)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_timetable.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    from pathplanning_amd._lib import TimetableParams, check, ptr
    from pathplanning_amd.planner import TIMETABLE_DTYPE, TIMETABLE_PLAN_DTYPE, TIMETABLE_STOP_DTYPE
    import speed_restatement as V
    import timetable_restatement as TT
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

    n, M = args.plans, args.max_stops
    lim = V.limits(spacing=float(np.float32(ms.resolution)), dwell=0.5)
    recs = pipe.speed_profile(tickets, max_samples=args.max_samples, samples=False, **lim)
    profiled = np.array([r.status == 0 for r in recs])
    duration, length = np.array([r.duration for r in recs]), np.array([r.s_last for r in recs])
    rng = np.random.RandomState(3)
    cases = {"one by arc length": ("length", (rng.uniform(0.0, 1.0, (n, 1)) * length[:, None]).copy()),
             "eight by time": ("time", (rng.uniform(-0.02, 1.02, (n, 8)) * duration[:, None]).copy())}
    print("fleet ready: %d plans, %d found, %d profiled" % (n, found, int(profiled.sum())), flush=True)

    c_tickets = np.ascontiguousarray(tickets, dtype=np.uint64)
    out = dict(tool="tools/bench_pipeline_timetable.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=n, plans_found=int(found), plans_profiled=int(profiled.sum()), max_stops=M, spacing=lim["spacing"], dwell=lim["dwell"], max_samples=args.max_samples,
               samples=int(sum(r.n_samples for r in recs)), reps=args.reps, host_reps=args.host_reps, device=torch.cuda.get_device_name(0), cases={})
    kept = {}
    for name, (by, values) in cases.items():
        P = values.shape[1]
        wrapped = pipe.timetable(tickets, values, by=by, max_stops=M)  # (untimed: the buffers are allocated here)
        c_plans, c_stops, c_out = np.zeros(n, dtype=TIMETABLE_PLAN_DTYPE), np.zeros((n, M), dtype=TIMETABLE_STOP_DTYPE), np.zeros((n, P), dtype=TIMETABLE_DTYPE)
        tp = TimetableParams(0 if by == "length" else 1, M)
        timed = {"c_abi": [], "wrapper": []}
        for rep in range(args.reps):
            t1 = time.perf_counter()
            check(pipe.lib.pp_pipeline_timetable(pipe.h, n, ptr(c_tickets), P, ptr(values), C.byref(tp), ptr(c_plans), ptr(c_stops), ptr(c_out)))
            timed["c_abi"].append(1e3 * (time.perf_counter() - t1))
            t1 = time.perf_counter()
            wrapped = pipe.timetable(tickets, values, by=by, max_stops=M)
            timed["wrapper"].append(1e3 * (time.perf_counter() - t1))
        same = bool(wrapped[0].tobytes() == c_plans.tobytes() and wrapped[1].tobytes() == c_stops.tobytes() and wrapped[2].tobytes() == c_out.tobytes())
        kept[name] = (c_plans.copy(), c_stops.copy(), c_out.copy())
        out["cases"][name] = dict(by=by, look_ups_per_plan=P, look_ups=n * P, stops_found=int(c_plans["n_stops"].sum()), stops_listed=int(c_plans["n_listed"].sum()),
                                  inside=int((c_out["status"] == 0).sum()), c_abi_equals_wrapper=same, bytes_down=int(c_plans.nbytes + c_stops.nbytes + c_out.nbytes),
                                  timetable_ms={k: stats(v) for k, v in timed.items()})
        print("%s: %.3f ms through the C ABI, %.3f ms through the wrapper, %d bytes down" % (name, np.median(timed["c_abi"]), np.median(timed["wrapper"]),
                                                                                       out["cases"][name]["bytes_down"]), flush=True)

    # ---- the host route: the rows down, then the same arithmetic in numpy (no pose: a host caller would need the path objects for it too)
    host = {name: dict(rows_ms=[], numpy_ms=[]) for name in cases}
    equal = {}
    for rep in range(args.host_reps):
        t1 = time.perf_counter()
        rows = pipe.speed_profile(tickets, max_samples=args.max_samples, samples=True, **lim)[1]
        rows_ms = 1e3 * (time.perf_counter() - t1)
        for name, (by, values) in cases.items():
            t1 = time.perf_counter()
            mine = [TT.timetable(False, r if len(r) else None, values[i], by, lim["a_acc"], lim["a_dec"], M) for i, r in enumerate(rows)]
            host[name]["rows_ms"].append(rows_ms)
            host[name]["numpy_ms"].append(1e3 * (time.perf_counter() - t1))
            if rep == 0:
                c_plans, c_stops, c_out = kept[name]
                ok = True
                for i, (rec, listed, want, _) in enumerate(mine):
                    ok &= rec.tobytes() == c_plans[i].tobytes() and listed.tobytes() == c_stops[i, :len(listed)].tobytes()
                    ok &= all(want[k].tobytes() == np.ascontiguousarray(c_out[i][k]).tobytes() for k in ("status", "row", "s", "t", "v", "a", "next_stop", "s_to_stop", "t_to_stop",
                                                                                                        "t_remaining"))
                equal[name] = bool(ok)
    rows_bytes = int(n * args.max_samples * 24)
    for name in cases:
        total = [a + b for a, b in zip(host[name]["rows_ms"], host[name]["numpy_ms"])]
        out["cases"][name]["host_route"] = dict(ms=stats(total), rows_ms=stats(host[name]["rows_ms"]), numpy_ms=stats(host[name]["numpy_ms"]), rows_bytes_down=rows_bytes,
                                                equals_the_call=equal[name])
        print("%s, host route: %.1f ms (%.1f ms of it the rows, %d bytes), equal to the call: %s" % (name, np.median(total), np.median(host[name]["rows_ms"]), rows_bytes,
                                                                                                    equal[name]), flush=True)
    pipe.speed_profile(tickets, max_samples=args.max_samples, samples=False, **lim)
    pipe.close()
    out["not_measured"] = ["the kernel's time apart from the call's", "a host route that forms the pose too", "more look-ups per plan than eight"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
