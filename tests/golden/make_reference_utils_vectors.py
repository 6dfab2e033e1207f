#!/usr/bin/env python3
"""Writes tests/golden/reference_utils.npz: what the reference's open list, grid neighbourhood, RNG and Modulo
(oracle/_ref/libppref.so, built by `make -C oracle ref` from the reference's sources) return for the inputs of
tests/ref_vectors.py.  Only inputs and returned numbers are stored.  Run from the repository root after the build."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_vectors as T  # noqa: E402


def ragged(arrays, dtype):
    off = np.cumsum([0] + [len(a) for a in arrays]).astype(np.int64)
    return np.concatenate([np.asarray(a, dtype=dtype).ravel() for a in arrays]) if arrays else np.zeros(0, dtype), off


def main():
    assert os.path.exists(T.REF_SO), "build oracle/_ref first (make -C oracle ref)"
    live = T.LiveReference(T.REF_SO)
    out = {}
    cases = T.frontier_cases()
    out["frontier_ops"], out["frontier_ops_offsets"] = ragged([o for o, _ in cases], np.int32)
    out["frontier_costs"], out["frontier_costs_offsets"] = ragged([c for _, c in cases], np.float64)
    out["frontier_popped"], out["frontier_popped_offsets"] = ragged([live.frontier_pops(i, o, c) for i, (o, c) in enumerate(cases)], np.int32)
    ncases = T.neighbor_cases()
    out["neighbor_cases"] = np.array(ncases, dtype=np.int32)
    rc = [live.neighbors(i, *c).ravel() for i, c in enumerate(ncases)]
    out["neighbor_rc"], off = ragged(rc, np.int32)
    out["neighbor_rc_offsets"] = off
    seeds, bounds, draws = [], [], []
    for seed in T.RNG_SEEDS:
        for lb, ub in T.RNG_BOUNDS:
            draws.append(live.rng_uniform(len(seeds), seed, T.RNG_DRAWS, lb, ub))
            seeds.append(seed)
            bounds.append((lb, ub))
    out["rng_seeds"] = np.array(seeds, dtype=np.uint64)
    out["rng_bounds"] = np.array(bounds)
    out["rng_uniform"] = np.array(draws)
    vals = T.modulo_values()
    out["modulo_in"] = vals
    out["modulo_out"] = np.array([live.modulo(i, float(v), 2 * np.pi) for i, v in enumerate(vals)])
    out["se2_uniform"], out["se2_gaussian"] = live.rng_se2(T.SE2_SEED, T.SE2_DRAWS, T.SE2_LB, T.SE2_UB, T.SE2_MEAN, T.SE2_STD)
    path = os.path.join(HERE, "reference_utils.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
