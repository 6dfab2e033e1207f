#!/usr/bin/env python3
"""What a heuristic clearance (include/pp_hip.h, "heuristic clearance") does to the search work on the benchmark's map -- on the CPU, with the
oracle (tests/oracle_lib.py), no GPU.  The benchmark's 1024^2 / 24-outline map (the oracle builds the same outlines and the reference's own
fields: oracle_lib.synthetic_world with the benchmark's seed), the first --queries of the benchmark's 4096 queries (its sampling: uniform
valid poses in reachable cells, seeds 1000 / 2000), each searched twice with oracle_lib.hybrid_batch on --threads threads: with the
reference's rule (clearance 0) and with clearance = minSafeRadius, which is the oracle on an occupancy grid that also holds every cell with
dist < minSafeRadius.  Records expansions, failures and cost changes.

    python tools/study_heuristic_clearance.py [--queries 512] [--threads 16] [--out profiles/heuristic_clearance_expansions.json]
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

import oracle_lib as O  # noqa: E402


def distance(w):
    return (np.sqrt(w.d2().astype(np.float64)) * np.float64(w.resolution)).astype(np.float32)  # gvd.h:38


def inflated_occupancy(w, radius):
    occ = w.occ()
    occ2 = np.where(distance(w) >= np.float32(radius), -1, 0).astype(np.int32)
    occ2[occ >= 0] = occ[occ >= 0]  # keep the original occupied ids
    return occ2


def reachable_mask(w, radius, seed=0):
    """pathplanning_amd.synthetic.reachable_mask on the CPU: the largest of four wavefronts over the occupancy inflated by the validator's radius"""
    tmp = O.World(float(w.ub[0]), float(w.ub[1]), float(w.resolution))
    tmp.set_occ(np.where(distance(w) < np.float32(radius), 0, -1).astype(np.int32))
    tmp.set_d2(w.d2())
    p = sample_valid_poses(w, 64, seed)
    fields = [tmp.obstacle_heuristic(g[:2])[0] for g in p[:4]]
    return np.isfinite(max(fields, key=lambda f: np.isfinite(f).sum()))


def sample_valid_poses(w, n, seed, reachable=None):
    """pathplanning_amd.synthetic.sample_valid_poses with the oracle's validator: the same draws, the same verdicts"""
    rng = np.random.RandomState(seed)
    out = np.empty((0, 3))
    res = float(w.resolution)
    while len(out) < n:
        k = 2 * (n - len(out)) + 64
        p = np.column_stack([rng.uniform(w.lb[0], w.ub[0], k), rng.uniform(w.lb[1], w.ub[1], k), rng.uniform(-math.pi, math.pi, k)])
        ok = w.is_state_valid(p).astype(bool)
        if reachable is not None:
            r = np.clip(((p[:, 0] - w.origin[0]) / res).astype(np.int64), 0, w.rows - 1)
            c = np.clip(((p[:, 1] - w.origin[1]) / res).astype(np.int64), 0, w.cols - 1)
            ok &= reachable[r, c]
        out = np.concatenate([out, p[ok]])
    return np.ascontiguousarray(out[:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--batch", type=int, default=4096, help="the benchmark's batch: its queries are sampled as one set of this size")
    ap.add_argument("--queries", type=int, default=512, help="how many of them, from the front")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heuristic_clearance_expansions.json"))
    args = ap.parse_args()

    t0 = time.time()
    w = O.synthetic_world(args.cells, args.obstacles, 1)
    radius = float(w.min_safe_radius)
    reach = reachable_mask(w, radius)
    n = args.queries
    starts = sample_valid_poses(w, args.batch, 1000, reach)[:n]
    goals = sample_valid_poses(w, args.batch, 2000, reach)[:n]
    seeds = np.arange(n, dtype=np.uint64)
    table, _ = O.nonholo_build(w.lb, w.ub, O.params_array(), threads=args.threads)
    print("map, queries and table: %.1f s" % (time.time() - t0), file=sys.stderr)

    secs0, status0, cost0, nexp0 = O.hybrid_batch(w, table, starts, goals, seeds, threads=args.threads)
    d2 = w.d2().copy()
    occ2 = inflated_occupancy(w, radius)
    n_occupied, n_blocked = int((w.occ() >= 0).sum()), int((occ2 >= 0).sum())
    w.set_occ(occ2)
    w.set_d2(d2)
    secs1, status1, cost1, nexp1 = O.hybrid_batch(w, table, starts, goals, seeds, threads=args.threads)

    both = (status0 == 0) & (status1 == 0)
    tol = 1e-9
    out = dict(tool="tools/study_heuristic_clearance.py",
               map="%d^2 cells, %d outline obstacles, seed 1 (the benchmark's map, built by the oracle)" % (args.cells, args.obstacles),
               queries="the first %d of the benchmark's %d (seeds 1000 / 2000, reachable cells)" % (n, args.batch), min_safe_radius=radius,
               blocked_cells=dict(reference_rule=n_occupied, clearance=n_blocked),
               expansions=dict(reference_rule=int(nexp0.sum()), clearance=int(nexp1.sum()), ratio=float(nexp0.sum() / max(1, nexp1.sum()))),
               expansions_max=dict(reference_rule=int(nexp0.max()), clearance=int(nexp1.max())),
               failures=dict(reference_rule=int((status0 != 0).sum()), clearance=int((status1 != 0).sum()),
                             fail_only_with_reference_rule=int(((status0 != 0) & (status1 == 0)).sum()),
                             fail_only_with_clearance=int(((status0 == 0) & (status1 != 0)).sum())),
               expansions_of_failures=dict(reference_rule=int(nexp0[status0 != 0].sum()), clearance=int(nexp1[status1 != 0].sum())),
               queries_whose_expansion_count_differs=int((nexp0 != nexp1).sum()),
               cost_where_both_succeed=dict(queries=int(both.sum()), lower_with_clearance=int((cost1[both] < cost0[both] - tol).sum()),
                                            higher_with_clearance=int((cost1[both] > cost0[both] + tol).sum()),
                                            equal=int((np.abs(cost1[both] - cost0[both]) <= tol).sum()),
                                            mean_relative_change=float(np.mean((cost1[both] - cost0[both]) / cost0[both])) if both.any() else 0.0),
               oracle_seconds=dict(reference_rule=float(secs0), clearance=float(secs1), threads=args.threads))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
