"""The numpy restatements of the exact-transform field mode (tests/gpu_common.py) against the CPU oracle, so that the -m gpu tests of
tests/test_gpu_fields_geometry.py rest on a checked reference.  CPU only.

  path_cost    PathCostMap::Update with the reference's float / double mix: bit-equal to the oracle's on the brushfire's own grids
  check_voro   CheckVoro over every neighbouring pair of FIXED labels: on the brushfire's final labels it reproduces the brushfire's
               own incremental Voronoi marks exactly
  exact_sq_edt the exact squared transform: equal to brute force, never above the brushfire's (which over-estimates a few cells)"""
import numpy as np
import pytest

import oracle_lib as O
from gpu_common import INT_MAX, brute_sq_edt, check_voro, exact_sq_edt, labels_are_nearest, path_cost
from test_gpu_fields_geometry import COST_PAIRS, FIELD_WORLDS, field_shapes


def oracle_world(name):
    spec = FIELD_WORLDS[name]
    w = O.World(lower=spec["lower"], upper=spec["upper"], resolution=spec["res"])
    for k, (kind, a, b, pose) in enumerate(field_shapes(name)):
        assert (w.add_rectangle(a, b, pose) if kind == "rect" else w.add_circle(a, b, pose)) == k
    assert (w.rows, w.cols) == spec["dims"]
    w.update()
    return w


@pytest.mark.parametrize("name", list(FIELD_WORLDS))
def test_path_cost_restatement_is_the_oracle_bit_for_bit(name):
    w = oracle_world(name)
    got = path_cost(w.d2(), w.voro_d2(), FIELD_WORLDS[name]["res"])
    want = w.pathcost()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (want > 0).mean() > 0.3
    # the zero branch: the restatement at a small d_max is zero exactly where the obstacle distance reaches it
    alpha, d_max = COST_PAIRS[1]
    small = path_cost(w.d2(), w.voro_d2(), FIELD_WORLDS[name]["res"], alpha, d_max)
    far = np.sqrt(w.d2().astype(np.float64)) * np.float64(np.float32(FIELD_WORLDS[name]["res"])) >= d_max
    assert (small[far] == 0).all() and (small[~far & (w.voro_d2() > 0)] > 0).all()


@pytest.mark.parametrize("name", list(FIELD_WORLDS))
def test_check_voro_on_the_brushfire_labels_is_the_brushfire(name):
    w = oracle_world(name)
    no, _ = O.world_nearest(w)
    occ = w.occ()
    d2 = w.d2().astype(np.int64)
    rr, cc = np.indices(d2.shape)
    assert np.array_equal((no[..., 0] - rr) ** 2 + (no[..., 1] - cc) ** 2, d2)  # the brushfire's d2 is its label's distance
    mark = check_voro(no, occ)
    want = w.voro_d2() == 0
    assert want.sum() > w.rows
    assert np.array_equal(mark, want), (int((mark & ~want).sum()), int((want & ~mark).sum()))


@pytest.mark.parametrize("name", list(FIELD_WORLDS))
def test_exact_transform_restatement(name):
    w = oracle_world(name)
    src = w.occ() >= 0
    exact = exact_sq_edt(src)
    assert (exact <= w.d2()).all()  # the brushfire's values are distances to obstacle cells
    assert (exact == w.d2()).mean() > 0.99
    if w.rows * w.cols <= 70000:
        assert np.array_equal(exact, brute_sq_edt(src))
    no, _ = O.world_nearest(w)
    assert labels_are_nearest(src, w.d2(), no)


def test_restatements_on_small_hand_made_grids():
    rng = np.random.RandomState(3)
    for shape in ((7, 11), (31, 5), (40, 40)):
        for p in (0.0, 0.01, 0.2):
            src = rng.rand(*shape) < p
            exact = exact_sq_edt(src)
            assert np.array_equal(exact, brute_sq_edt(src))
            if not src.any():
                assert (exact == INT_MAX).all()
    # two vertical walls of different ids, 9 columns apart: the two middle columns are the edge, marked from both sides
    occ = np.full((12, 13), -1, np.int32)
    occ[:, 2], occ[:, 11] = 0, 1
    rr, cc = np.indices(occ.shape)
    labels = np.stack([rr, np.where(cc <= 6, 2, 11)], -1).astype(np.int32)  # column 6: 4 from the left wall; column 7: 4 from the right
    assert labels_are_nearest(occ >= 0, np.minimum((cc - 2) ** 2, (cc - 11) ** 2), labels)
    mark = check_voro(labels, occ)
    assert np.array_equal(np.nonzero(mark.any(0))[0], [6, 7]) and mark[:, 6].all() and mark[:, 7].all()
    # the same walls with one id: nothing
    assert not check_voro(labels, np.where(occ >= 0, 0, -1)).any()
    # a label one cell off is not a nearest label
    bad = labels.copy()
    bad[5, 5] = [5, 11]
    assert not labels_are_nearest(occ >= 0, np.minimum((cc - 2) ** 2, (cc - 11) ** 2), bad)
