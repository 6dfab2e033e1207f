#!/usr/bin/env python3
"""What it costs to give a fleet's held plans waits at their start or at their stops that clear their conflicts: the fleet of
tools/bench_pipeline_deconflict.py -- ONE pipeline on the benchmark's 1024^2 synthetic map, --plans queries searched and HELD and given a speed
profile, every plan paired with its --nearest nearest plans by start pose, a --horizon s horizon at dt = --dt, waits of up to --max-delay-steps lattice
steps, priority = the index of a plan.  In one process:
  the figure to compare with:  pp_pipeline_deconflict into an array that exists, --reps times;
  library call:  pp_pipeline_deconflict_waits into an array that exists (what a C or C++ caller pays), --reps times, for each max_places of --places and
                 once more at the largest one with every vehicle barred from its start;
  wrapper call:  pa.HybridAStarPipeline.deconflict_waits, which returns one numpy record array, --reps times each (fewer, and recorded, where --reps pairs of
                 calls would take longer than --config-budget seconds);
  host route:    what a caller could do before the call existed -- conflicts(poses=True) over the extended horizon, the stops of timetable() with their
                 standing poses looked up by arc length, the arrive columns and the rule in numpy, vehicle after vehicle and candidate after candidate
                 -- once, at --host-places places, and given up after --host-budget seconds; the vehicles it decided are compared with the call's.
Host clock around each; median and spread of the repetitions.  At max_places = 0 the records' shared fields are asserted equal to deconflict's.

    python tools/bench_pipeline_deconflict_waits.py [--plans 4096] [--nearest 32] [--horizon 60] [--dt 0.1] [--max-delay-steps 300] [--places 0,4,16] [--reps 7]
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


def host_route(pipe, tickets, t_start, pairs, kw, D, P, radius, budget):
    """the records' (status, place, wait_steps) by the host route, for the vehicles decided within `budget` seconds: (decided, status, place, steps, ms)"""
    t1 = time.perf_counter()
    n, dt = len(tickets), kw["dt"]
    k0 = int(np.ceil(kw["t_from"] / dt))
    T = int(np.floor(kw["t_to"] / dt)) - k0 + 1
    wider = dict(kw, t_from=(k0 - D - 0.5) * dt)
    poses = np.asarray(pipe.conflicts(tickets, t_start, pairs=np.zeros((0, 2), dtype=np.int32), poses=True, **wider)[2])[:, :, :2]  # [n, T + D, 2]
    plans, stops, _ = pipe.timetable(tickets, np.zeros((n, 1)), by="time", max_stops=64)
    tau = (np.arange(T + D) + float(k0 - D)) * np.float64(dt)
    below = [[] for _ in range(n)]
    for a, b in pairs.tolist():
        below[max(a, b)].append(min(a, b))
    spots = []
    for i in range(n):  # the places: inner stops reached inside the horizon, the first P, with the pose at their arc length
        mine = []
        if plans[i].status == 0:
            u = tau - np.float64(t_start[i])
            for st in stops[i][:plans[i].n_listed]:
                at = np.flatnonzero(u >= st.t_arrive)
                a = int(at[0]) if len(at) else T + D
                if 0 < st.row < plans[i].n_samples - 1 and D <= a < T + D and len(mine) < P:
                    mine.append((a, float(st.s)))
        spots.append(mine)
    wanted = np.zeros((n, max(P, 1)))
    for i, mine in enumerate(spots):
        wanted[i, :len(mine)] = [s for _, s in mine]
    looked = pipe.timetable(tickets, wanted, by="length", max_stops=0)[2].pose[:, :, :2]  # [n, P, 2]
    standing = [looked[i, :len(mine)] for i, mine in enumerate(spots)]
    m = np.arange(T) + D
    comp = [None] * n
    decided = np.zeros(n, dtype=bool)
    status, place, steps = np.full(n, -1), np.full(n, -2), np.full(n, -1)
    for i in range(n):
        if time.perf_counter() - t1 > budget:
            break
        decided[i] = True
        if plans[i].status != 0:
            continue
        partners = [comp[j] for j in sorted(set(below[i])) if comp[j] is not None]
        theirs = np.stack(partners) if partners else None
        status[i] = 1
        tried = [(-2, 0)] + [c for d in range(1, D + 1) for c in [(-1, d)] + [(q, d) for q in range(len(spots[i]))]]
        for q, d in tried:
            if q == -1:
                mine = poses[i][m - d]
            elif q >= 0:
                a = spots[i][q][0]
                mine = np.where((m < a)[:, None], poses[i][m], np.where((m < a + d)[:, None], standing[i][q][None], poses[i][m - d]))
            else:
                mine = poses[i][m]
            if theirs is None or not (np.sqrt(((theirs - mine[None]) ** 2).sum(axis=2)) - 2.0 * radius < kw["margin"]).any():  # (NaN compares false: absent)
                status[i], place[i], steps[i], comp[i] = 0, q, d, mine
                break
    return decided, status, place, steps, 1e3 * (time.perf_counter() - t1)


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
    ap.add_argument("--places", default="0,4,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--config-budget", type=float, default=40.0, help="seconds of timed calls per configuration: fewer than --reps repetitions are made (at least one) if one call is long")
    ap.add_argument("--host-places", type=int, default=4)
    ap.add_argument("--host-budget", type=float, default=60.0, help="seconds after which the host route is given up")
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_deconflict_waits.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    from pathplanning_amd._lib import ConflictParams, DelayParams, WaitParams, check, ptr
    from pathplanning_amd.planner import DELAY_DTYPE, WAIT_DTYPE, delay_levels
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
    lim = V.limits(spacing=float(np.float32(ms.resolution)))
    pairs = nearest_pairs(starts, args.nearest)
    t_start = np.round(np.random.RandomState(3).uniform(0.0, 0.5 * args.horizon, n), 3) + 0.0123
    kw = dict(t_from=0.0, t_to=args.horizon, dt=dt, margin=args.margin, hold_after=True)
    n_levels = int(delay_levels(n, pairs).max()) + 1
    profiled = pipe.speed_profile(tickets, max_samples=args.max_samples, samples=False, **lim)
    cusp_stops = int(sum(r.n_cusps for r in profiled if r.status == 0))

    c_tickets, c_starts = np.ascontiguousarray(tickets, dtype=np.uint64), np.ascontiguousarray(t_start, dtype=np.float64)
    lattice = ConflictParams(kw["t_from"], kw["t_to"], dt, args.margin, 0, 1)
    d_params, d_out = DelayParams(lattice, D, 0), np.zeros(n, dtype=DELAY_DTYPE)
    plain = []
    for rep in range(-1, args.reps):  # rep -1: warmed, untimed (the buffers are allocated there)
        t1 = time.perf_counter()
        check(pipe.lib.pp_pipeline_deconflict(pipe.h, n, ptr(c_tickets), ptr(c_starts), len(pairs), ptr(pairs), C.byref(d_params), ptr(d_out)))
        if rep >= 0:
            plain.append(1e3 * (time.perf_counter() - t1))

    barred = np.ones(n, dtype=np.uint8)
    configs = [(int(p), False) for p in args.places.split(",")]
    configs.append((configs[-1][0], True))
    calls, kept = [], {}
    for P, no_start in configs:
        w_params, w_out = WaitParams(d_params, P, 0), np.zeros(n, dtype=WAIT_DTYPE)
        flags = barred if no_start else None
        timed = {"c_abi": [], "wrapper": []}
        wrapped = None
        reps = args.reps
        for rep in range(-1, args.reps):
            if rep >= reps:
                break
            t1 = time.perf_counter()
            check(pipe.lib.pp_pipeline_deconflict_waits(pipe.h, n, ptr(c_tickets), ptr(c_starts), ptr(flags), None, len(pairs), ptr(pairs), C.byref(w_params), None, None, ptr(w_out)))
            if rep >= 0:
                timed["c_abi"].append(1e3 * (time.perf_counter() - t1))
            t1 = time.perf_counter()
            wrapped = pipe.deconflict_waits(tickets, t_start, pairs=pairs, no_start_wait=flags, max_delay_steps=D, max_places=P, **kw)
            if rep >= 0:
                timed["wrapper"].append(1e3 * (time.perf_counter() - t1))
            else:  # (the warm pair of calls says how many timed pairs fit the budget)
                reps = max(1, min(args.reps, int(args.config_budget / max(time.perf_counter() - t1, 1e-3) / 2.0)))
        assert wrapped.tobytes() == w_out.tobytes()
        if P == 0 and not no_start:
            for mine, theirs in (("status", "status"), ("wait_steps", "delay_steps"), ("n_tried", "n_tried"), ("blocker", "blocker"), ("t_start", "t_start"), ("t_block", "t_block"),
                                 ("s_block", "s_block")):
                assert w_out[mine].tobytes() == d_out[theirs].tobytes(), mine
        kept[(P, no_start)] = w_out.copy()
        calls.append(dict(max_places=P, no_start_wait=no_start, reps=reps, ms={k: stats(v) for k, v in timed.items()},
                          factor_over_deconflict=float(np.median(timed["c_abi"]) / np.median(plain)),
                          scheduled=int((w_out["status"] == 0).sum()), waiting_at_the_start=int((w_out["place"] == -1).sum()), waiting_at_a_stop=int((w_out["place"] >= 0).sum()),
                          without_a_clear_candidate=int((w_out["status"] == 1).sum()), without_a_plan=int((w_out["status"] == -1).sum()),
                          candidates_tried=int(w_out["n_tried"].astype(np.int64).sum())))

    host = None
    if (args.host_places, False) in kept:
        radius = float(val.min_safe_radius)
        decided, status, place, steps, host_ms = host_route(pipe, tickets, t_start, pairs, kw, D, args.host_places, radius, args.host_budget)
        device = kept[(args.host_places, False)]
        same = (status[decided] == device["status"][decided]) & (place[decided] == device["place"][decided]) & (steps[decided] == device["wait_steps"][decided])
        host = dict(max_places=args.host_places, ms=host_ms, finished=bool(decided.all()), vehicles_decided=int(decided.sum()), records_that_differ_from_the_calls=int((~same).sum()))
    pipe.close()

    out = dict(tool="tools/bench_pipeline_deconflict_waits.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=n, plans_found=int(found), nearest=args.nearest, pairs=int(len(pairs)), levels=n_levels, lattice_times=int(round(args.horizon / dt)) + 1, horizon=args.horizon,
               dt=dt, margin=args.margin, hold_after=True, max_delay_steps=D, reps=args.reps, spacing=lim["spacing"], device=torch.cuda.get_device_name(0), cusp_stops=cusp_stops,
               deconflict_c_abi_ms=stats(plain), deconflict_waits=calls, host_route=host,
               not_measured=["each kernel's time apart from the call's", "the calls without the shortcut (no switch turns it off)", "a multi-disc footprint at this scale",
                             "fixed waits at this scale", "the host route repeated, or at other place counts"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
