#!/usr/bin/env python3
"""What it costs to give a fleet's held plans speeds and arrival times: ONE pipeline on the benchmark's 1024^2 synthetic map, --plans queries
searched and HELD, then, in the same process, two routes to the same profiles:
  speed profile: one pp_pipeline_speed_profile call over every held ticket (k_speed_profile_tickets, one wave per plan), spacing = the map's
                 resolution, whole plans from rest to rest -- without the clearance term, with it, and records only (no sample rows copied back),
                 --reps times each;
  host route:    what a caller could do before that call existed -- get_path_of per ticket (one blocking copy of the slot's records each), the edges
                 rebuilt on the host (arcs from the closed form in numpy; the Reeds-Shepp edge through pp_rs_connect and pp_rs_path_interpolate), the
                 rule of include/pp_hip.h evaluated in numpy (tests/speed_restatement.py, the comparator of the GPU test), the clearance term from the
                 map's downloaded distance grid (tests/footprint_ref.py) -- --host-reps times each, without and with the clearance term.
Host clock around each route; median of the repetitions and their spread.  The two routes' profiles are compared under the rule of
tests/test_gpu_pipeline_speed_profile.py: status, n_samples, n_cusps and length equal, s equal bit for bit, v equal bit for bit at decided samples and
within 1e-12 relative at the others, t within 1e-9 relative.

    python tools/bench_pipeline_speed_profile.py [--plans 4096] [--reps 7] [--host-reps 3] [--out profiles/pipeline_speed_profile.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# the pipeline runs although its streams may share hardware queues (the runtime's own number of queues is left as the environment has it)
os.environ.setdefault("PP_PIPE_ALLOW_SHARED_QUEUES", "1")

GAIN, FLOOR = 1.5, 0.3


class HostGrid:
    """what tests/footprint_ref.py reads of a map: bounds, geometry and the float distance grid, downloaded"""

    def __init__(self, ms):
        self.lb, self.ub = ms.lower, ms.upper
        self.rows, self.cols = ms.rows, ms.cols
        self.origin = ms.grid_origin
        self.resd = np.float64(ms.resolution)
        self.dist = ms.download_distance()


def host_plan(R, feed, pipe, rs, prims, ticket, status, goal):
    """the host route's first half: the plan of a held ticket as edge objects (None: no plan); as tools/bench_pipeline_locate.py builds it, and the
    Reeds-Shepp record carries the plan's own t, u, v (the connection solved again may differ in the last bits, which choose the motion at a boundary)"""
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
            if rec["word"][0] == prim:
                for k, f in enumerate(feed[prim // 4]):
                    rec["motion_length"][0][k] = (p["tuv"][e][0], p["tuv"][e][1], p["tuv"][e][2], math.pi / 2)[f]
            rec["length"][0] = L  # (the plan's own bits: arc lengths are sums of these)
            edges.append(R.RsEdge(rec, L, rs.interpolate))
    return R.Plan(p["poses"][0], edges)


def stats(ms_list):
    return dict(median=float(np.median(ms_list)), min=float(min(ms_list)), max=float(max(ms_list)), runs=[float(x) for x in ms_list])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--plans", type=int, default=4096, help="held plans (= the pipeline's capacity)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_speed_profile.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    import locate_restatement as R
    import speed_restatement as V
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
    spacing = float(np.float32(ms.resolution))
    free, near = V.limits(spacing=spacing), V.limits(spacing=spacing, clearance_gain=GAIN, v_floor=FLOOR)
    discs = [(0.0, 0.0, float(np.float32(val.min_safe_radius)))]

    timed = {"without_clearance": [], "with_clearance": [], "records_only": []}
    device = {}
    for rep in range(-1, args.reps):  # rep -1: warmed, untimed (the buffers are allocated there)
        for name, lim, samples in (("without_clearance", free, True), ("with_clearance", near, True), ("records_only", free, False)):
            t1 = time.perf_counter()
            device[name] = pipe.speed_profile(tickets, max_samples=args.max_samples, samples=samples, **lim)
            if rep >= 0:
                timed[name].append(1e3 * (time.perf_counter() - t1))
    host_ms = {"without_clearance": [], "with_clearance": []}
    host = {}
    for rep in range(args.host_reps):
        for name, lim in (("without_clearance", free), ("with_clearance", near)):
            t1 = time.perf_counter()
            clearance = V.grid_clearance(HostGrid(ms), discs) if lim["clearance_gain"] > 0.0 else None
            host[name] = [V.profile(host_plan(R, RS_FEED, pipe, rs, prims, t, status[q], goals[q]), lim, max_samples=args.max_samples, clearance=clearance) for q, t in enumerate(tickets)]
            host_ms[name].append(1e3 * (time.perf_counter() - t1))
    pipe.close()

    agreement = {}
    for name in host:
        recs, rows = device[name]
        profiled = samples = undecided = wrong = 0
        for a, r, b in zip(recs, rows, host[name]):
            if (a.status, a.n_samples, a.n_cusps) != (b["status"], b["n_samples"], b["n_cusps"]) or a.length != b["length"]:
                wrong += 1
                continue
            if b["status"] != 0:
                continue
            profiled += 1
            samples += b["n_samples"]
            undecided += int((~b["decided"]).sum())
            same_v = r[:, 1].view(np.uint64) == b["v"].view(np.uint64)
            ok = np.array_equal(r[:, 0].view(np.uint64), b["s"].view(np.uint64)) and (same_v | ~b["decided"]).all()
            ok = ok and (np.abs(r[:, 1] - b["v"]) <= 1e-12 * np.abs(b["v"])).all() and (np.abs(r[:, 2] - b["t"]) <= 1e-9 * np.abs(b["t"])).all()
            wrong += not ok
        agreement[name] = dict(profiled=profiled, samples=samples, undecided_samples=undecided, records_that_disagree=int(wrong))

    out = dict(tool="tools/bench_pipeline_speed_profile.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=args.plans, plans_found=sum(s == 0 for s in status), reps=args.reps, host_reps=args.host_reps, spacing=spacing, max_samples=args.max_samples,
               clearance_term=dict(gain=GAIN, v_floor=FLOOR, discs=discs), device=torch.cuda.get_device_name(0), agreement=agreement,
               speed_profile_ms={k: stats(v) for k, v in timed.items()}, host_route_ms={k: stats(v) for k, v in host_ms.items()},
               ratio_host_route_over_speed_profile={k: float(np.median(host_ms[k]) / np.median(timed[k])) for k in host_ms})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert all(a["records_that_disagree"] == 0 for a in agreement.values()), "the two routes disagree: %r" % agreement


if __name__ == "__main__":
    main()
