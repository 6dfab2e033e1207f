#!/usr/bin/env python3
"""What it costs to find a fleet's vehicles on the plans a pipeline holds: ONE pipeline on the benchmark's 1024^2 synthetic map, --plans queries
searched and HELD, one vehicle pose per plan near the plan (a point of the plan at a random arc length, pushed sideways by up to 0.5 m and turned by
up to 0.3 rad), then, in the same process, two routes to the same records, --reps times each:
  locate:      one pp_pipeline_locate call over every held ticket (k_locate_tickets, one wave per plan), spacing = the map's resolution;
  host route:  what a caller could do before that call existed -- get_path_of per ticket (one blocking copy of the slot's records each), the edges
               rebuilt on the host (arcs from the closed form in numpy; the Reeds-Shepp edge through pp_rs_connect and pp_rs_path_interpolate),
               the two stages of include/pp_hip.h evaluated in numpy (tests/locate_restatement.py, the comparator of the GPU test).
Host clock around each route; median of --reps and their spread.  The two routes' records are compared under the rule of
tests/test_gpu_pipeline_locate.py: status, n_samples and length equal; on a decided case edge, direction and s equal and the rest within 1e-9; on an
undecided one the cost of the device's (edge, ratio) within 1e-9 m^2 of the host's minimum.

    python tools/bench_pipeline_locate.py [--plans 4096] [--reps 7] [--out profiles/pipeline_locate.json]
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

# the pipeline runs although its streams may share hardware queues (the runtime's own number of queues is left as the environment has it)
os.environ.setdefault("PP_PIPE_ALLOW_SHARED_QUEUES", "1")

TOL = 1e-9
FIELDS = ("ratio", "distance", "along", "lateral", "heading_error")


def host_plan(R, pipe, rs, prims, ticket, status, goal):
    """the host route's first half: the plan of a held ticket as edge objects (None: no plan)"""
    if status != 0:
        return None
    _, curv, direc = prims
    p = pipe.get_path_of(ticket)
    edges = []
    for e in range(1, len(p["poses"])):
        L, prim = float(p["length"][e]), int(p["prim"][e])
        if p["kind"][e] == 1:
            edges.append(R.ArcEdge(p["poses"][e - 1], L, curv[prim], direc[prim]))
        else:
            rec = rs.connect(p["poses"][e - 1][None], np.asarray(goal)[None])
            rec["length"][0] = L  # (the plan's own bits: arc lengths are sums of these)
            edges.append(R.RsEdge(rec, L, rs.interpolate))
    return R.Plan(p["poses"][0], edges)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--plans", type=int, default=4096, help="held plans (= the pipeline's capacity)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--heading-weight", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_locate.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    import locate_restatement as R
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
    spacing, w = float(np.float32(ms.resolution)), args.heading_weight
    # one vehicle per plan, near the plan (untimed)
    rng = np.random.RandomState(5)
    half = 0.5 * args.cells * spacing
    vehicles = np.array([R.vehicle_poses(host_plan(R, pipe, rs, prims, t, status[q], goals[q]), starts[q], goals[q], half, rng, n_random=1)[0] for q, t in enumerate(tickets)])

    new_ms, old_ms, device, host = [], [], None, None
    for rep in range(-1, args.reps):  # rep -1: both routes warmed, untimed
        t1 = time.perf_counter()
        device = pipe.locate(tickets, vehicles, spacing=spacing, heading_weight=w)
        dt_new = time.perf_counter() - t1
        t1 = time.perf_counter()
        host = [R.locate(host_plan(R, pipe, rs, prims, t, status[q], goals[q]), vehicles[q], spacing, w) for q, t in enumerate(tickets)]
        dt_old = time.perf_counter() - t1
        if rep >= 0:
            new_ms.append(1e3 * dt_new)
            old_ms.append(1e3 * dt_old)
    pipe.close()

    located = undecided = wrong = 0
    worst = 0.0
    for a, b in zip(device, host):
        if (a.status, a.n_samples) != (b["status"], b["n_samples"]) or a.length != b["length"]:
            wrong += 1
            continue
        if b["status"] != 0:
            continue
        located += 1
        if not b["decided"]:
            undecided += 1
            wrong += abs(b["cost_at"](a.edge, a.ratio) - b["c"]) > TOL
            continue
        diff = max([abs(getattr(a, f) - b[f]) for f in FIELDS] + [abs(x - y) for x, y in zip(a.pose, b["pose"])])
        worst = max(worst, diff)
        wrong += (a.edge, a.direction) != (b["edge"], b["direction"]) or a.s != b["s"] or diff > TOL

    out = dict(tool="tools/bench_pipeline_locate.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=args.plans, plans_found=sum(s == 0 for s in status), reps=args.reps, spacing=spacing, heading_weight=w, device=torch.cuda.get_device_name(0),
               samples=sum(r.n_samples for r in device), located=located, undecided=undecided, records_that_disagree=int(wrong), largest_difference_on_a_decided_case=worst,
               locate_ms=dict(median=float(np.median(new_ms)), min=float(min(new_ms)), max=float(max(new_ms)), runs=new_ms),
               host_route_ms=dict(median=float(np.median(old_ms)), min=float(min(old_ms)), max=float(max(old_ms)), runs=old_ms),
               ratio_host_route_over_locate=float(np.median(old_ms) / np.median(new_ms)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert wrong == 0, "the two routes disagree on %d records" % wrong


if __name__ == "__main__":
    main()
