"""Pins the oracle's open list, neighbour order and RNG to the REFERENCE'S OWN CODE: oracle/_ref/libppref.so where it is built,
its recorded answers (tests/golden/reference_utils.npz) elsewhere -- see tests/ref_vectors.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from ref_vectors import (GOLDEN, REF_SO, RNG_BOUNDS, RNG_DRAWS, RNG_SEEDS, SE2_DRAWS, SE2_LB, SE2_MEAN, SE2_SEED, SE2_STD, SE2_UB, LiveReference,
                         RecordedReference, frontier_cases, modulo_values, neighbor_cases, reference)


@pytest.fixture(scope="module")
def ref():
    return reference()


def test_pop_order_matches_reference_frontier(ref):
    for trial, (ops, costs) in enumerate(frontier_cases()):
        want = ref.frontier_pops(trial, ops, costs)
        assert len(want) == len(costs)
        assert np.array_equal(O.frontier_replay(ops, costs, 0), want)  # (cost,-seq) heap
        assert np.array_equal(O.frontier_replay(ops, costs, 1), want)  # literal restatement


def test_reference_test_frontier_binary_passes():
    exe = os.path.join(O.ORACLE_DIR, "_ref", "test_frontier")
    if not os.path.exists(exe):
        pytest.skip("reference test binary not built")
    assert subprocess.call([exe]) == 0


def test_neighbor_order_matches_reference(ref):
    for i, (r, c, rows, cols) in enumerate(neighbor_cases()):
        mine = O.neighbors(r, c, rows, cols)
        assert np.array_equal(mine, ref.neighbors(i, r, c, rows, cols)), (r, c, rows, cols)


def test_rng_matches_reference_random(ref):
    i = 0
    for seed in RNG_SEEDS:
        for lb, ub in RNG_BOUNDS:
            out = ref.rng_uniform(i, seed, RNG_DRAWS, lb, ub)
            assert np.array_equal(O.rng_uniform(seed, RNG_DRAWS, lb, ub), out)
            i += 1


def test_modulo_matches_reference(ref):
    for i, v in enumerate(modulo_values()):
        m = ref.modulo(i, float(v), 2 * math.pi)
        x = math.fmod(v, 2 * math.pi)
        if x < 0:
            x += 2 * math.pi
        assert m == x


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs the reference's sources)")
def test_recorded_vectors_match_the_reference_build():
    """tests/golden/reference_utils.npz holds exactly what libppref.so returns for this module's inputs."""
    live, rec = LiveReference(REF_SO), RecordedReference(GOLDEN)
    for i, (ops, costs) in enumerate(frontier_cases()):
        assert np.array_equal(live.frontier_pops(i, ops, costs), rec.frontier_pops(i, ops, costs))
    for i, case in enumerate(neighbor_cases()):
        assert np.array_equal(live.neighbors(i, *case), rec.neighbors(i, *case))
    i = 0
    for seed in RNG_SEEDS:
        for lb, ub in RNG_BOUNDS:
            assert np.array_equal(live.rng_uniform(i, seed, RNG_DRAWS, lb, ub), rec.rng_uniform(i, seed, RNG_DRAWS, lb, ub))
            i += 1
    for i, v in enumerate(modulo_values()):
        assert live.modulo(i, float(v), 2 * math.pi) == rec.modulo(i, float(v), 2 * math.pi)
    args = (SE2_SEED, SE2_DRAWS, SE2_LB, SE2_UB, SE2_MEAN, SE2_STD)
    assert all(np.array_equal(a, b) for a, b in zip(live.rng_se2(*args), rec.rng_se2(*args)))
