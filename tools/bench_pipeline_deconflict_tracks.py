#!/usr/bin/env python3
"""What it costs to give a fleet's held plans start delays that clear their conflicts AND a set of tracked movers: the configuration of
tools/bench_pipeline_deconflict.py -- ONE pipeline on the benchmark's 1024^2 synthetic map, --plans queries searched and HELD and given a speed profile,
every plan paired with its --nearest nearest plans by start pose, a --horizon s horizon at dt = --dt, delays of up to --max-delay-steps lattice steps,
priority = the index of a plan -- plus --tracks movers: discs of radius 0, 0.3 and 1.0 m that drive at 1.5 m/s on straight lines between start poses of
the fleet, each from a time of its own inside the horizon.  Then, in the same process, three routes to the delays:
  library call:  pp_pipeline_deconflict_tracks into arrays that exist (what a C or C++ caller pays) -- the levels and partner lists on the host, the track
                 samples (k_track_samples), the extended trajectory (k_trajectory_tickets), one k_delay_level_tracks launch per level and k_track_pairs
                 behind the last -- --reps times;
  wrapper call:  pa.HybridAStarPipeline.deconflict_tracks, which returns two numpy record arrays, --reps times;
  host route:    what a caller could do before the call existed -- conflicts(poses=True) over the horizon that begins max_delay_steps steps earlier brings
                 the extended trajectory down, and a numpy loop applies the rule: vehicles in index order, delays ascending, the scheduled partners of
                 smaller index and every track at all lattice times of a candidate at once -- once, and given up after --host-budget seconds.
Host clock around each; median and spread of the repetitions.  The host route works on the device's own poses and a delay is an index shift, so its
delays are the call's; the vehicles whose delay differs are counted, not asserted.  The three kernels' registers and scratch come from
tools/kernel_resources.py.  These are measurements to report, not thresholds.

    python tools/bench_pipeline_deconflict_tracks.py [--plans 4096] [--nearest 32] [--tracks 64] [--horizon 60] [--dt 0.1] [--max-delay-steps 300] [--reps 7]
                                                     [--out profiles/pipeline_deconflict_tracks.json]
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

KERNELS = ("k_track_samples", "k_delay_level_tracks", "k_track_pairs")


def stats(ms_list):
    return dict(median=float(np.median(ms_list)), min=float(min(ms_list)), max=float(max(ms_list)), runs=[float(x) for x in ms_list])


def movers(starts, count, horizon, seed=5):
    """`count` tracks [(radius, waypoints [2, 3])]: straight lines between two start poses of the fleet at 1.5 m/s, from a time of their own on"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        a, b = rng.choice(len(starts), 2, replace=False)
        t0 = float(np.round(rng.uniform(0.0, 0.6 * horizon), 3)) + 0.0071
        length = float(np.hypot(*(starts[b][:2] - starts[a][:2])))
        out.append(((0.0, 0.3, 1.0)[k % 3], np.array([[t0, *starts[a][:2]], [t0 + max(length / 1.5, 1.0), *starts[b][:2]]])))
    return out


def sampled(tracks, tau):
    """[M, T, 2] positions on the lattice, NaN where absent: the header's interpolation"""
    out = np.full((len(tracks), len(tau), 2), np.nan)
    for k, (_, w) in enumerate(tracks):
        there = (tau >= w[0, 0]) & (tau <= w[-1, 0])
        j = np.clip(np.searchsorted(w[:, 0], tau, side="right") - 1, 0, len(w) - 1)
        j1 = np.minimum(j + 1, len(w) - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = (tau - w[j, 0]) / (w[j1, 0] - w[j, 0])
            x = np.where(j == len(w) - 1, w[j, 1], w[j, 1] + lam * (w[j1, 1] - w[j, 1]))
            y = np.where(j == len(w) - 1, w[j, 2], w[j, 2] + lam * (w[j1, 2] - w[j, 2]))
        out[k, there, 0], out[k, there, 1] = x[there], y[there]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1024)
    ap.add_argument("--obstacles", type=int, default=24)
    ap.add_argument("--plans", type=int, default=4096, help="held plans (= the pipeline's capacity)")
    ap.add_argument("--nearest", type=int, default=32)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--horizon", type=float, default=60.0)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--margin", type=float, default=0.5)
    ap.add_argument("--max-delay-steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-budget", type=float, default=150.0, help="seconds after which the host route's loop is given up")
    ap.add_argument("--pipe-rows", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=81920)
    ap.add_argument("--max-samples", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_deconflict_tracks.json"))
    args = ap.parse_args()

    import torch
    import pathplanning_amd as pa
    from pathplanning_amd import build, synthetic
    from pathplanning_amd._lib import ConflictParams, DelayParams, check, ptr
    from pathplanning_amd.planner import DELAY_DTYPE, TRACK_DTYPE, conflict_lattice, delay_levels, track_set
    import kernel_resources
    import speed_restatement as V
    from bench_pipeline_conflicts import nearest_pairs
    assert torch.cuda.is_available(), "needs a GPU"
    resources = {k["kernel"]: {f: k[f] for f in ("vgpr", "sgpr", "scratch_bytes_per_lane", "vgpr_spill", "lds_bytes")} for k in kernel_resources.resources(build.LIB)
                 if k["kernel"] in KERNELS}
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

    n, D, dt, M = args.plans, args.max_delay_steps, args.dt, args.tracks
    lim = V.limits(spacing=float(np.float32(ms.resolution)))
    pairs = nearest_pairs(starts, args.nearest)
    t_start = np.round(np.random.RandomState(3).uniform(0.0, 0.5 * args.horizon, n), 3) + 0.0123
    kw = dict(t_from=0.0, t_to=args.horizon, dt=dt, margin=args.margin, hold_after=True)
    tracks = movers(np.asarray(starts), M, args.horizon)
    level = delay_levels(n, pairs)
    n_levels = int(level.max()) + 1
    pipe.speed_profile(tickets, max_samples=args.max_samples, samples=False, **lim)

    c_tickets, c_starts = np.ascontiguousarray(tickets, dtype=np.uint64), np.ascontiguousarray(t_start, dtype=np.float64)
    c_params = DelayParams(ConflictParams(kw["t_from"], kw["t_to"], dt, args.margin, 0, 1), D, 0)
    c_tracks, keep = track_set(tracks)
    c_out, c_rec = np.zeros(n, dtype=DELAY_DTYPE), np.zeros((n, M), dtype=TRACK_DTYPE)
    timed = {"c_abi": [], "c_abi_without_track_records": [], "wrapper": []}
    wrapped = None
    for rep in range(-1, args.reps):  # rep -1: warmed, untimed (the buffers are allocated there)
        t1 = time.perf_counter()
        check(pipe.lib.pp_pipeline_deconflict_tracks(pipe.h, n, ptr(c_tickets), ptr(c_starts), len(pairs), ptr(pairs), C.byref(c_params), C.byref(c_tracks), ptr(c_out), ptr(c_rec)))
        if rep >= 0:
            timed["c_abi"].append(1e3 * (time.perf_counter() - t1))
        t1 = time.perf_counter()
        check(pipe.lib.pp_pipeline_deconflict_tracks(pipe.h, n, ptr(c_tickets), ptr(c_starts), len(pairs), ptr(pairs), C.byref(c_params), C.byref(c_tracks), ptr(c_out), None))
        if rep >= 0:
            timed["c_abi_without_track_records"].append(1e3 * (time.perf_counter() - t1))
        t1 = time.perf_counter()
        wrapped = pipe.deconflict_tracks(tickets, t_start, tracks, pairs=pairs, max_delay_steps=D, **kw)
        if rep >= 0:
            timed["wrapper"].append(1e3 * (time.perf_counter() - t1))
    assert wrapped[0].tobytes() == c_out.tobytes() and wrapped[1].tobytes() == c_rec.tobytes()
    device = c_out.copy()
    plain = pipe.deconflict(tickets, t_start, pairs=pairs, max_delay_steps=D, **kw)  # the same fleet without the movers, for the figures below

    # ---- the host route: the extended trajectory down, then the rule in numpy
    k0, T = conflict_lattice(kw["t_from"], kw["t_to"], dt)
    tau = np.array([float(k0 + i) for i in range(T)]) * np.float64(dt)
    R = float(np.float32(val.min_safe_radius))
    t1 = time.perf_counter()
    wider = dict(kw, t_from=(k0 - D - 0.5) * dt)
    assert conflict_lattice(wider["t_from"], wider["t_to"], dt) == (k0 - D, T + D)
    plan_recs, _, poses = pipe.conflicts(tickets, t_start, pairs=np.zeros((0, 2), dtype=np.int32), poses=True, **wider)
    download_ms = 1e3 * (time.perf_counter() - t1)
    xy = np.stack([p[:, :2] for p in poses])  # [n, T + D, 2], NaN where absent
    del poses
    track_xy = sampled(tracks, tau)
    track_r = np.array([r for r, _ in tracks])[:, None]
    below = [[] for _ in range(n)]
    for a, b in pairs.tolist():
        below[max(a, b)].append(min(a, b))
    delay = np.full(n, -2, dtype=np.int64)  # -2: not decided yet; -1: no clear delay, or no plan
    tried = 0
    finished = True
    m_all = np.arange(T)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            if plan_recs[i].status < 0:
                delay[i] = -1
                continue
            partners = sorted({j for j in below[i] if delay[j] >= 0})
            others = np.stack([xy[j, m_all + D - delay[j]] for j in partners]) if partners else np.zeros((0, T, 2))
            delay[i] = -1
            for d in range(D + 1):
                mine = xy[i, m_all + D - d]
                tried += 1
                # (a comparison with a NaN is false: absent vehicles and tracks are never in conflict)
                if ((np.hypot(others[:, :, 0] - mine[:, 0], others[:, :, 1] - mine[:, 1]) - (R + R)) < args.margin).any():
                    continue
                if ((np.hypot(track_xy[:, :, 0] - mine[:, 0], track_xy[:, :, 1] - mine[:, 1]) - (R + track_r)) < args.margin).any():
                    continue
                delay[i] = d
                break
            if time.perf_counter() - t1 > args.host_budget:
                finished = False
                break
    host_ms = 1e3 * (time.perf_counter() - t1)
    pipe.close()
    del keep

    decided = delay > -2
    differ = int((delay[decided] != device["delay_steps"][decided]).sum())
    by_track = device["blocker"] >= n
    out = dict(tool="tools/bench_pipeline_deconflict_tracks.py", map="%d^2 cells, %d outline obstacles (the benchmark's synthetic map, exact-transform fields)" % (args.cells, args.obstacles),
               held_plans=n, plans_found=int(found), nearest=args.nearest, pairs=int(len(pairs)), levels=n_levels, largest_level=int(np.bincount(level).max()), tracks=M,
               lattice_times=int(T), horizon=args.horizon, dt=dt, margin=args.margin, hold_after=True, max_delay_steps=D, reps=args.reps,
               spacing=lim["spacing"], device=torch.cuda.get_device_name(0),
               scheduled=int((device["status"] == 0).sum()), waiting=int((device["delay_steps"] > 0).sum()), without_a_clear_delay=int((device["status"] == 1).sum()),
               without_a_plan=int((device["status"] == -1).sum()), longest_delay_steps=int(device["delay_steps"].max()), candidates_tried=int(device["n_tried"].sum()),
               last_rejected_by_a_track=int(by_track.sum()), last_rejected_by_a_vehicle=int(((device["blocker"] >= 0) & ~by_track).sum()),
               track_records=dict(conflict=int((c_rec["status"] == 1).sum()), clear=int((c_rec["status"] == 0).sum()), never_both_present=int((c_rec["status"] == 2).sum())),
               without_the_tracks=dict(waiting=int((plain["delay_steps"] > 0).sum()), without_a_clear_delay=int((plain["status"] == 1).sum()),
                                       candidates_tried=int(plain["n_tried"].sum()), delays_that_differ=int((plain["delay_steps"] != device["delay_steps"]).sum())),
               deconflict_tracks_ms={k: stats(v) for k, v in timed.items()},
               host_route=dict(ms=host_ms, of_which_conflicts_with_poses_ms=download_ms, finished=finished, vehicles_decided=int(decided.sum()), candidates_tried=int(tried),
                               delays_that_differ_from_the_calls=differ, same_delays=bool(finished and differ == 0)),
               ratio_host_route_over_c_abi=float(host_ms / np.median(timed["c_abi"])) if finished else None,
               kernels=resources,
               not_measured=["each kernel's time apart from the call's", "a multi-disc footprint at this scale", "more tracks than 64 (the call is O(n (D + 1) T M) at worst)",
                             "the host route repeated (it runs once)"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
