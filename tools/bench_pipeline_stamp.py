#!/usr/bin/env python3
"""What it costs to turn the plans a pipeline holds into a reservation map: ONE pipeline on the benchmark's 1024^2 synthetic map, --plans
queries searched and HELD, then, in the same process and for two vehicle shapes (the point validator's disc, which is the benchmark's
footprint-free default, and a three-disc footprint), two routes to the same grid in a SECOND map of the context, --reps times each:
  stamp:       one pp_pipeline_stamp call over every held ticket (k_stamp_tickets, one wave per plan), spacing = the map's resolution;
  round trip:  what a caller could do before that call existed -- get_path_of per ticket (one blocking copy of the slot's records each), the
               edges sampled on the host (arcs in numpy from the closed form; the Reeds-Shepp edge through pp_rs_connect and
               pp_rs_path_interpolate, one call each over all plans), the discs rasterised in numpy (row spans per disc centre, merged
               with a difference array: no per-cell loop), the covered cells pushed through pp_map_set_cells.
Host clock around each route; median of --reps and their spread.  The two resulting grids are compared under the undecided-cell rule of
tests/test_gpu_pipeline_stamp.py: with EPS = 1e-7 m a cell is decided-in if some disc sample has dist <= R - EPS, decided-out if all have
dist > R + EPS; every decided cell of both grids must hold what the rule says.

    python tools/bench_pipeline_stamp.py [--plans 4096] [--reps 7] [--out profiles/pipeline_stamp.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the pipeline runs although its streams may share hardware queues (the runtime's own number of queues is left as the environment has it)
os.environ.setdefault("PP_PIPE_ALLOW_SHARED_QUEUES", "1")

EPS = 1e-7
VALUE = 1


def sample_plans(pipe, rs, prims, tickets, results, goals, spacing):
    """the host route's first half: [m, 3] sample poses of every held plan (junction poses twice, as the stamp samples them)"""
    _, curv, direc = prims
    poses, rs_from, rs_goal, rs_len = [], [], [], []
    for q, t in enumerate(tickets):
        if results[q]["status"] != 0:
            continue
        p = pipe.get_path_of(t)
        n_path = len(p["poses"])
        if n_path == 1:
            poses.append(p["poses"][:1])
        for e in range(1, n_path):
            L = float(p["length"][e])
            n = int(math.ceil(L / spacing)) if L > 0 else 0
            if p["kind"][e] == 1:
                ratio = np.arange(n + 1) / n if n else np.zeros(1)
                x0, y0, t0 = p["poses"][e - 1]
                kappa, d = curv[int(p["prim"][e])], L * ratio
                if direc[int(p["prim"][e])]:
                    d = -d
                if abs(kappa) > 1e-9:
                    th = t0 + d * kappa
                    poses.append(np.column_stack([x0 + 1 / kappa * (np.sin(th) - math.sin(t0)), y0 + 1 / kappa * (-np.cos(th) + math.cos(t0)), th]))
                else:
                    poses.append(np.column_stack([x0 + d * math.cos(t0), y0 + d * math.sin(t0), np.full(len(d), t0)]))
            else:
                rs_from.append(p["poses"][e - 1])
                rs_goal.append(goals[q])
                rs_len.append(n)
    if rs_from:
        rec = rs.connect(np.array(rs_from), np.array(rs_goal))
        reps = np.array(rs_len) + 1
        ratio = np.concatenate([np.arange(n + 1) / n if n else np.zeros(1) for n in rs_len])
        poses.append(rs.interpolate(np.repeat(rec, reps), ratio)[0])
    return np.concatenate(poses)


def covered(ms, poses, discs, margin, shrink=0.0):
    """bool [rows, cols]: cells whose centre lies within r + margin - shrink of some disc centre; row spans merged through a difference array"""
    rows, cols, res = ms.rows, ms.cols, float(np.float32(ms.resolution))
    gx, gy = float(ms.grid_origin[0]), float(ms.grid_origin[1])
    diff = np.zeros(rows * (cols + 1), dtype=np.int64)
    s, c = np.sin(poses[:, 2]), np.cos(poses[:, 2])
    for ox, oy, r in discs:
        R = float(np.float32(r)) + float(np.float32(margin)) - shrink
        cx, cy = (poses[:, 0] + ox * c) - oy * s, (poses[:, 1] + ox * s) + oy * c
        h = int(math.ceil(R / res)) + 1
        base = np.floor((cx - gx) / res).astype(np.int64)
        for k in range(-h, h + 1):
            row = base + k
            dx = (gx + (row + 0.5) * res) - cx
            h2 = R * R - dx * dx
            ok = (h2 >= 0) & (row >= 0) & (row < rows)
            half = np.sqrt(h2[ok])
            lo = np.ceil((cy[ok] - half - gy) / res - 0.5).astype(np.int64)
            hi = np.floor((cy[ok] + half - gy) / res - 0.5).astype(np.int64)
            lo, hi = np.maximum(lo, 0), np.minimum(hi, cols - 1)
            keep = lo <= hi
            at = row[ok][keep] * (cols + 1)
            diff += np.bincount(at + lo[keep], minlength=len(diff)) - np.bincount(at + hi[keep] + 1, minlength=len(diff))
    return np.cumsum(diff.reshape(rows, cols + 1), axis=1)[:, :cols] > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--plans", type=int, default=4096, help="held plans (= the pipeline's capacity)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_stamp.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import synthetic
    from pathplanning_amd._lib import ptr
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

    rs = pa.ReedsSheppPaths(ctx, params.min_turning_radius, params.direction_switching_cost, params.reverse_cost_multiplier, params.forward_cost_multiplier)
    prims = params.primitives()
    spacing = float(np.float32(ms.resolution))
    lib = pipe.lib
    lib.pp_map_set_cells.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
    shapes = [("point validator's disc", None, [(0.0, 0.0, float(val.min_safe_radius))], 0.0),
              ("three-disc footprint, cover_rectangle(4.0, 1.8, 1.0, 3), margin 0.12", pa.Footprint.cover_rectangle(ms, 4.0, 1.8, 1.0, 3), None, 0.12)]
    cases = []
    for name, fp, discs, margin in shapes:
        pipe.set_footprint(fp)
        discs = fp.discs if fp is not None else discs
        new_ms, old_ms, stamped, pushed, n_samples = [], [], None, None, 0
        for rep in range(-1, args.reps):  # rep -1: both routes warmed, untimed
            target = pa.OccupancyMapSet.from_bounds(ctx, m["lower"], m["upper"], m["resolution"])
            target.upload_occupancy(np.full((ms.rows, ms.cols), -1, dtype=np.int32))
            t1 = time.perf_counter()
            records = pipe.stamp(tickets, map_set=target, values=VALUE, spacing=spacing, margin=margin)
            dt_new = time.perf_counter() - t1
            stamped = target.download_occupancy()
            n_samples = sum(r.n_samples for r in records)
            target.close()
            target = pa.OccupancyMapSet.from_bounds(ctx, m["lower"], m["upper"], m["resolution"])
            target.upload_occupancy(np.full((ms.rows, ms.cols), -1, dtype=np.int32))
            t1 = time.perf_counter()
            poses = sample_plans(pipe, rs, prims, tickets, results, goals, spacing)
            cells = np.ascontiguousarray(np.argwhere(covered(target, poses, discs, margin)), dtype=np.int32)
            rc = lib.pp_map_set_cells(target.h, len(cells), ptr(cells), VALUE)
            dt_old = time.perf_counter() - t1
            assert rc == 0
            pushed = target.download_occupancy()
            target.close()
            if rep >= 0:
                new_ms.append(1e3 * dt_new)
                old_ms.append(1e3 * dt_old)
        assert len(poses) == n_samples, (len(poses), n_samples)
        inn, out = covered(ms, poses, discs, margin, shrink=EPS), ~covered(ms, poses, discs, margin, shrink=-EPS)
        bad_new = int(((stamped != VALUE) & inn).sum() + ((stamped != -1) & out).sum())
        bad_old = int(((pushed != VALUE) & inn).sum() + ((pushed != -1) & out).sum())
        cases.append(dict(shape=name, discs=len(discs), margin=margin, samples=n_samples, cells_decided_in=int(inn.sum()), cells_undecided=int((~inn & ~out).sum()),
                          stamp_ms=dict(median=float(np.median(new_ms)), min=float(min(new_ms)), max=float(max(new_ms)), runs=new_ms),
                          round_trip_ms=dict(median=float(np.median(old_ms)), min=float(min(old_ms)), max=float(max(old_ms)), runs=old_ms),
                          ratio_round_trip_over_stamp=float(np.median(old_ms) / np.median(new_ms)),
                          decided_cells_wrong_in_the_stamped_grid=bad_new, decided_cells_wrong_in_the_round_trip_grid=bad_old))
    pipe.set_footprint(None)
    pipe.close()

    out = dict(tool="tools/bench_pipeline_stamp.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=args.plans, plans_found=sum(r["status"] == 0 for r in results), reps=args.reps, spacing=spacing, device=torch.cuda.get_device_name(0), cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert all(c["decided_cells_wrong_in_the_stamped_grid"] == 0 and c["decided_cells_wrong_in_the_round_trip_grid"] == 0 for c in cases), "the two routes disagree"


if __name__ == "__main__":
    main()
