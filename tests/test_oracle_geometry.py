"""The oracle helpers for worlds off the default geometry (tests/test_gpu_geometry.py): explicit state boxes, the grid they size and
where it lies, and the instrumentation count of the negative-k table reads.  CPU only."""
import math

import numpy as np

import oracle_lib as O


def test_symmetric_signature_is_the_explicit_box():
    a = O.World(12.8, 6.4, 0.1)
    b = O.World(lower=(-12.8, -6.4), upper=(12.8, 6.4), resolution=0.1)
    assert np.array_equal(a.lb, b.lb) and np.array_equal(a.ub, b.ub)
    assert (a.rows, a.cols) == (b.rows, b.cols) == (256, 128)
    assert np.array_equal(a.origin, b.origin)
    assert np.array_equal(a.lb, [-12.8, -6.4, -math.pi]) and np.array_equal(a.ub, [12.8, 6.4, math.pi])


def test_off_centre_box_sizes_a_grid_centred_on_the_local_origin():
    """occupancy_map.cpp:6-14 via state_validator_occupancy_map.cpp:6-13: float width / height of the box, grid origin -width / 2"""
    w = O.World(lower=(-7.3, -20.1), upper=(18.9, 4.4), resolution=0.1)
    assert (w.rows, w.cols) == (262, 245)
    width, height = np.float32(18.9 - -7.3), np.float32(4.4 - -20.1)
    assert np.array_equal(w.origin, [-float(width) / 2.0, -float(height) / 2.0])
    assert np.array_equal(w.grid_hi, w.origin + np.array([262, 245]) * float(np.float32(0.1)))
    w.update()
    # in the box but off the grid, and in the grid but outside the box: both invalid; the overlap is free
    probe = np.array([[16.0, -5.0, 0.0], [0.0, -15.0, 0.0], [-10.0, -5.0, 0.0], [0.0, 8.0, 0.0], [0.0, -5.0, 0.0]])
    assert w.is_state_valid(probe).tolist() == [0, 0, 0, 0, 1]
    assert w.to_cell(probe[:1, :2]).tolist() == [[-1, -1]]


def test_synthetic_world_bounds_form_places_obstacles_in_the_grid():
    for lower, upper, res in (((-16.65, -10.0), (16.65, 10.0), 0.1), ((-7.3, -20.1), (18.9, 4.4), 0.1), ((-12.15, -15.0), (12.15, 15.0), 0.15)):
        w = O.synthetic_world(0, 10, 3, res, lower=lower, upper=upper)
        occ = w.occ() >= 0
        assert 0.002 < occ.mean() < 0.1
        rows = np.nonzero(occ.any(axis=1))[0]
        cols = np.nonzero(occ.any(axis=0))[0]
        assert rows.min() > 0 and rows.max() < w.rows - 1 and cols.min() > 0 and cols.max() < w.cols - 1
    # the square form is the one it always was
    a, b = O.synthetic_world(128, 4, 9), O.synthetic_world(128, 4, 9)
    assert np.array_equal(a.occ(), b.occ()) and (a.rows, a.cols) == (128, 128)


def test_negative_k_stride_reads_are_counted():
    """NonHolonomicHeuristic::Lookup's reads of row j-1 through the heap-chunk stride (k <= -2): counted per search, for odd and even
    numbers of heading bins, and none in the wrapped-bin mode"""
    w = O.synthetic_world(0, 6, 5, 0.1, lower=(-16.65, -10.0), upper=(16.65, 10.0))
    rng = np.random.RandomState(4)
    starts, goals = [], []
    while len(starts) < 6:
        p = np.column_stack([rng.uniform(-15, 15, 2), rng.uniform(-9, 9, 2), rng.uniform(-math.pi, math.pi, 2)])
        if w.is_state_valid(p).all():
            starts.append(p[0])
            goals.append(p[1])
    for kw, na in ((dict(spatial_resolution=2.0, angular_resolution=0.0875), 72), ({}, 73)):
        params = O.params_array(**kw)
        h = O.Hybrid(w, params)
        assert h.table.shape[2] == na
        reads = [h.search(s, g, 3)["n_negative_k_stride_reads"] for s, g in zip(starts, goals)]
        assert sum(reads) > 0, (na, reads)
        again = [h.search(s, g, 3)["n_negative_k_stride_reads"] for s, g in zip(starts, goals)]
        assert again == reads  # reset per search
        off = O.Hybrid(w, params, negative_k_read=False, table=h.table)
        assert all(off.search(s, g, 3)["n_negative_k_stride_reads"] == 0 for s, g in zip(starts, goals))
