#!/usr/bin/env python3
"""What it costs to ask whether the plans a pipeline holds are still collision-free after the map changed: ONE pipeline on the benchmark's
1024^2 synthetic map, --plans queries searched and HELD, a few walls added on the device and the fields rebuilt (pp_map_update_gvd), then,
in the same process, two routes to the same verdicts, --reps times each:
  revalidate:  one pp_pipeline_revalidate call over every held ticket (k_revalidate_tickets, one wave per plan);
  round trip:  what a caller could do before that call existed -- get_path_of per ticket (one blocking copy of the slot's records each),
               the edges rebuilt on the host (arcs from the primitive index, the Reeds-Shepp edge through pp_rs_connect), then
               pp_check_arcs, pp_check_rs_paths and pp_check_states over all of them.
Host clock around each route; median of --reps and their spread.  The two routes' verdicts (status and first blocked edge) are compared.

    python tools/bench_pipeline_revalidate.py [--plans 4096] [--reps 7] [--out profiles/pipeline_revalidate.json]
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


def round_trip(pa, pipe, val, rs, prims, tickets, results, goals_of):
    """the host route: -> [(status, first blocked edge)] per ticket"""
    _, curv, direc = prims
    arc_from, arc_prim, arc_len, arc_at, rs_from, rs_goal, rs_at, last, last_at, n_edges = [], [], [], [], [], [], [], [], [], {}
    for q, t in enumerate(tickets):
        if results[q]["status"] != 0:
            continue
        p = pipe.get_path_of(t)
        n = len(p["poses"])
        n_edges[q] = n - 1
        last.append(p["poses"][-1])
        last_at.append(q)
        for e in range(1, n):
            if p["kind"][e] == 1:
                arc_from.append(p["poses"][e - 1])
                arc_prim.append(int(p["prim"][e]))
                arc_len.append(p["length"][e])
                arc_at.append((q, e))
            else:
                rs_from.append(p["poses"][e - 1])
                rs_goal.append(goals_of[q])
                rs_at.append((q, e))
    arc_prim = np.array(arc_prim, dtype=np.int64)
    blocked = {}
    if arc_at:
        ok, _ = val.is_path_valid(np.array(arc_from), curv[arc_prim], np.array(arc_len), direc[arc_prim])
        for i in np.nonzero(~ok)[0]:
            q, e = arc_at[i]
            blocked[q] = min(blocked.get(q, e), e)
    if rs_at:
        ok, _ = val.is_rs_path_valid(rs.connect(np.array(rs_from), np.array(rs_goal)))
        for i in np.nonzero(~ok)[0]:
            q, e = rs_at[i]
            blocked[q] = min(blocked.get(q, e), e)
    goal_ok = dict(zip(last_at, val.is_state_valid(np.array(last)))) if last_at else {}
    out = []
    for q in range(len(tickets)):
        if q not in n_edges:
            out.append((-1, 0))
        elif q in blocked:
            out.append((1, blocked[q]))
        else:
            out.append((0 if goal_ok[q] else 2, 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--plans", type=int, default=4096, help="held plans (= the pipeline's capacity)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--walls", type=int, default=12, help="12 m x 0.5 m walls added after the searches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_revalidate.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
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
    results = [None] * args.plans
    t0 = time.perf_counter()
    done = 0
    while done < args.plans:
        got, res = pipe.poll(4096, release=False)
        for k, t in enumerate(got):
            results[index_of[int(t)]] = dict(status=res[k].status, n_path=res[k].n_path)
        done += len(got)
        if time.perf_counter() - t0 > 600:
            raise RuntimeError("pipeline stalled: %d of %d results" % (done, args.plans))
    # the map changes with nothing in flight: walls on the device, fields rebuilt
    rng = np.random.RandomState(3)
    half = 0.5 * args.cells * 0.1
    for k in range(args.walls):
        pose = (rng.uniform(-0.8 * half, 0.8 * half), rng.uniform(-0.8 * half, 0.8 * half), rng.uniform(-np.pi, np.pi))
        ms.add_polygon([(6.0, 0.25), (-6.0, 0.25), (-6.0, -0.25), (6.0, -0.25)], pose, args.obstacles + k)
    t1 = time.perf_counter()
    ms.update_gvd()
    update_ms = 1e3 * (time.perf_counter() - t1)

    rs = pa.ReedsSheppPaths(ctx, params.min_turning_radius, params.direction_switching_cost, params.reverse_cost_multiplier, params.forward_cost_multiplier)
    prims = params.primitives()
    new_ms, old_ms, new, old = [], [], None, None
    for rep in range(-1, args.reps):  # rep -1: both routes warmed, untimed
        t1 = time.perf_counter()
        new = pipe.revalidate(tickets)
        dt_new = time.perf_counter() - t1
        t1 = time.perf_counter()
        old = round_trip(pa, pipe, val, rs, prims, tickets, results, goals)
        dt_old = time.perf_counter() - t1
        if rep >= 0:
            new_ms.append(1e3 * dt_new)
            old_ms.append(1e3 * dt_old)
    agree = sum((r.status, r.blocked_edge) == o for r, o in zip(new, old))
    pipe.close()

    out = dict(tool="tools/bench_pipeline_revalidate.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields), %d walls added" %
               (args.cells, args.obstacles, args.walls), held_plans=args.plans, plans_found=sum(r["status"] == 0 for r in results), reps=args.reps,
               device=torch.cuda.get_device_name(0), field_update_ms=update_ms,
               revalidate_ms=dict(median=float(np.median(new_ms)), min=float(min(new_ms)), max=float(max(new_ms)), runs=new_ms),
               round_trip_ms=dict(median=float(np.median(old_ms)), min=float(min(old_ms)), max=float(max(old_ms)), runs=old_ms),
               ratio_round_trip_over_revalidate=float(np.median(old_ms) / np.median(new_ms)),
               statuses={str(k): sum(r.status == k for r in new) for k in (-4, -1, 0, 1, 2)}, verdicts_equal=agree)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert agree == args.plans, "the two routes disagree on %d plans" % (args.plans - agree)


if __name__ == "__main__":
    main()
