#!/usr/bin/env python3
"""Footprint state checks/s and arc checks/s for K = 1, 3, 5 discs next to pp_check_states / pp_check_arcs on the same device-resident
inputs in the same process (1024^2 synthetic map).  K = 1 is the point disc {(0, 0, minSafeRadius)} (the point validator's verdicts);
K = 3, 5 are pp_footprint_cover_rectangle(4.8, 2.0, 1.0, K) (one radius, one bitmap).

Method: inputs generated on the device from a seed; every kernel warmed up; per repetition the point check and each footprint are
timed one after the other (alternating, so drift hits all alike) with HIP events on the library's stream around `inner` back-to-back
launches; the median over the repetitions is reported, with the spread (min, max).  Rates are whole-call rates (launch included).

  python tools/bench_footprint.py [--states N] [--arcs M] [--reps R] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pathplanning_amd as pa  # noqa: E402
from pathplanning_amd import synthetic  # noqa: E402
from pathplanning_amd._lib import check  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1 << 24)
    ap.add_argument("--arcs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pa.Context(0)
    m = synthetic.make_map(1024, 24, seed=1)
    ms, val = synthetic.upload(ctx, m)
    lib = ctx.lib
    half = float(m["upper"][0])
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    n, na = a.states, a.arcs
    poses = torch.empty(n, 3, dtype=torch.float64, device=dev)
    poses[:, 0].uniform_(-half, half, generator=g)
    poses[:, 1].uniform_(-half, half, generator=g)
    poses[:, 2].uniform_(-math.pi, math.pi, generator=g)
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    frm = poses[:na].contiguous()
    _, curv, direc = pa.HybridAStarSearchParameters().primitives()
    pick = torch.randint(0, len(curv), (na,), generator=g, device=dev)
    kappa = torch.from_numpy(curv).to(dev)[pick].contiguous()
    direction = torch.from_numpy(direc).to(dev)[pick].contiguous()
    length = torch.full((na,), 3.0, dtype=torch.float64, device=dev)
    avalid = torch.empty(na, dtype=torch.uint8, device=dev)
    alast = torch.empty(na, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    fps = {1: pa.Footprint(ms, [(0.0, 0.0, val.min_safe_radius)]), 3: pa.Footprint.cover_rectangle(ms, 4.8, 2.0, 1.0, 3), 5: pa.Footprint.cover_rectangle(ms, 4.8, 2.0, 1.0, 5)}

    def states(fp):
        if fp is None:
            check(lib.pp_check_states_dev(ms.h, n, p(poses), p(out)))
        else:
            check(lib.pp_check_states_footprint_dev(ms.h, fp.h, n, p(poses), p(out)))

    def arcs(fp):
        if fp is None:
            check(lib.pp_check_arcs_dev(ms.h, na, p(frm), p(kappa), p(length), p(direction), p(avalid), p(alast)))
        else:
            check(lib.pp_check_arcs_footprint_dev(ms.h, fp.h, na, p(frm), p(kappa), p(length), p(direction), p(avalid), p(alast)))

    def measure(fn, count):
        cases = [("point", None)] + [("K=%d" % k, fps[k]) for k in (1, 3, 5)]
        share = {}
        for name, fp in cases:  # warm-up of every kernel, and the verdicts
            for _ in range(2):
                fn(fp)
            ctx.synchronize()
            share[name] = float((out if fn is states else avalid).float().mean().item())
        times = {name: [] for name, _ in cases}
        for _ in range(a.reps):
            for name, fp in cases:
                ctx.timer_start()
                for _ in range(a.inner):
                    fn(fp)
                times[name].append(ctx.timer_stop() / a.inner)
        res = {}
        for name, _ in cases:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(ms_median=med, ms_min=min(t), ms_max=max(t), checks_per_s=count / (med * 1e-3), valid_share=share[name])
        for name in ("K=1", "K=3", "K=5"):
            res[name]["rate_vs_point"] = res[name]["checks_per_s"] / res["point"]["checks_per_s"]
        return res

    result = dict(map="synthetic 1024^2, 24 obstacles, seed 1", n_states=n, n_arcs=na, arc_length=3.0,
                  reps=a.reps, inner=a.inner, device=torch.cuda.get_device_name(0), states=measure(states, n), arcs=measure(arcs, na))
    assert result["states"]["K=1"]["valid_share"] == result["states"]["point"]["valid_share"]
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
