"""CPU side of the vehicle footprint (include/pp_hip.h, "vehicle footprint"): the C ABI is exported, the rectangle cover is right,
the numpy restatement (tests/footprint_ref.py) with the footprint {(0, 0, minSafeRadius)} IS the oracle's point validator, and the
new kernels' register / scratch figures.  No GPU needed."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import footprint_ref as R  # noqa: E402
import oracle_lib as O  # noqa: E402

NEW_SYMBOLS = ["pp_footprint_create", "pp_footprint_destroy", "pp_footprint_cover_rectangle", "pp_check_states_footprint", "pp_check_states_footprint_dev",
               "pp_check_arcs_footprint", "pp_check_arcs_footprint_dev", "pp_check_rs_paths_footprint", "pp_check_rs_paths_footprint_dev",
               "pp_check_se2_paths_footprint", "pp_planner_set_footprint"]

PP_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from pathplanning_amd import build
    return C.CDLL(build.build(verbose=False))


def test_footprint_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert "#define PP_FOOTPRINT_MAX_DISCS 8" in header
    for s in NEW_SYMBOLS:
        assert s + "(" in header, s
        assert hasattr(lib, s), s


def _cover(lib, length, width, rear, n):
    from pathplanning_amd._lib import FootprintDisc
    arr = (FootprintDisc * 8)()
    lib.pp_footprint_cover_rectangle.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int32, C.c_void_p]
    rc = lib.pp_footprint_cover_rectangle(length, width, rear, n, arr)
    return rc, [(arr[i].ox, arr[i].oy, arr[i].r) for i in range(max(0, min(n, 8)))]


def test_cover_rectangle_follows_the_formula_and_covers(lib):
    length, width, rear = 4.8, 2.0, 1.0
    xs = np.arange(-rear, length - rear + 1e-12, 0.05)
    ys = np.arange(-width / 2, width / 2 + 1e-12, 0.05)
    gx, gy = np.meshgrid(np.append(xs, length - rear), np.append(ys, width / 2))  # (the far edges too)
    for n in range(1, 9):
        rc, discs = _cover(lib, length, width, rear, n)
        assert rc == 0 and len(discs) == n
        s = length / n
        want_r = math.sqrt((s / 2) ** 2 + (width / 2) ** 2)
        for i, (ox, oy, r) in enumerate(discs):
            assert ox == -rear + (i + 0.5) * s and oy == 0.0
            assert r == float(np.float32(r)) and r >= want_r and float(np.nextafter(np.float32(r), np.float32(0))) < want_r  # rounded UP to float, by at most one ulp
        assert discs == R.cover_rectangle(length, width, rear, n)
        inside = np.zeros(gx.shape, bool)
        for ox, oy, r in discs:
            inside |= (gx - ox) ** 2 + (gy - oy) ** 2 <= r * r
        assert inside.all(), n


def test_cover_rectangle_rejects_bad_arguments(lib):
    lib.pp_last_error.restype = C.c_char_p
    for args in ((4.8, 2.0, 1.0, 0), (4.8, 2.0, 1.0, 9), (4.8, 2.0, 1.0, -1), (0.0, 2.0, 1.0, 3), (-1.0, 2.0, 1.0, 3), (4.8, 0.0, 1.0, 3), (4.8, -2.0, 1.0, 3),
                 (float("nan"), 2.0, 1.0, 3), (4.8, float("inf"), 1.0, 3), (4.8, 2.0, float("nan"), 3)):
        rc, _ = _cover(lib, *args)
        assert rc == PP_ERR_INVALID, args
        assert lib.pp_last_error(), args
    lib.pp_footprint_cover_rectangle.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int32, C.c_void_p]
    assert lib.pp_footprint_cover_rectangle(4.8, 2.0, 1.0, 3, None) == PP_ERR_INVALID


@pytest.mark.parametrize("n_cells,n_obstacles,seed", [(256, 6, 3), (512, 12, 3)])
def test_restatement_with_the_point_disc_is_the_oracle(n_cells, n_obstacles, seed):
    """pins the yardstick, not the feature: {(0, 0, 1.0)} against World.is_state_valid and World.is_path_valid_csteer, flags and
    `last` with float equality, no exclusions"""
    from pathplanning_amd.planner import HybridAStarSearchParameters
    w = O.synthetic_world(n_cells, n_obstacles, seed)
    g = R.Grid(w)
    discs = [(0.0, 0.0, 1.0)]
    rng = np.random.RandomState(100 + n_cells)
    poses = R.continuous_poses(rng, w, 200000)
    ok, _, _, guard = R.fp_state(g, poses, discs)
    assert np.array_equal(ok, w.is_state_valid(poses).astype(bool))
    assert 0.2 < ok.mean() < 0.95
    assert guard.mean() <= R.MAX_LEFT_OUT
    steer, curv, _ = HybridAStarSearchParameters().primitives()
    for backward in (0, 1):
        n = 20000
        frm = R.continuous_poses(rng, w, n, margin=1.0)
        pick = rng.randint(0, len(steer), n)
        length = rng.choice([1.5, 0.0, 3.0, 7.5], n, p=[0.6, 0.02, 0.28, 0.1])
        v, last, guard, samples = R.fp_arcs(g, frm, curv[pick], length, backward, discs)
        v_want, l_want = w.is_path_valid_csteer(frm, steer[pick], length, np.full(n, backward, np.int32))
        assert np.array_equal(v, v_want.astype(bool))
        assert np.array_equal(last, l_want)
        assert 0.2 < v.mean() < 0.95
        assert guard.mean() <= R.MAX_LEFT_OUT


def test_restatement_rs_and_se2_with_the_point_disc_are_the_oracle():
    w = O.synthetic_world(256, 6, 3)
    g = R.Grid(w)
    discs = [(0.0, 0.0, 1.0)]
    rng = np.random.RandomState(7)
    n = 4000
    a = R.continuous_poses(rng, w, n, margin=0.95)
    b = a.copy()
    b[:, :2] += rng.uniform(-6, 6, (n, 2))
    b[:, 2] = rng.uniform(-1.2 * math.pi, 1.2 * math.pi, n)
    paths = O.rs_connect(a, b, 2.0)
    v, last, _, _ = R.fp_rs_paths(g, paths, discs)
    v_want, l_want = O.rs_paths_valid(w, paths)
    assert np.array_equal(v, v_want) and np.array_equal(last, l_want)
    assert 0.1 < v.mean() < 0.95
    v, last, _, _ = R.fp_se2_paths(g, a, b, discs)
    v_want, l_want = O.se2_paths_valid(w, a, b)
    assert np.array_equal(v, v_want) and np.array_equal(last, l_want)
    assert 0.1 < v.mean() < 0.95


# kernel -> (max scratch bytes per lane, max VGPR spills).  State and path kernels: no scratch and no spills, like their point counterparts;
# the Reeds-Shepp one like k_check_rs_paths, whose 112 B are rs::Path's indexed motion arrays, not spills.  The search kernel: the figures of the
# build this test was written against (k_hybrid_search<false> next to it: 112 B, 0 spills).
LIMITS = {
    "k_check_states_footprint": (0, 0),
    "k_check_states_footprint_pipe": (0, 0),
    "k_check_arcs_footprint": (0, 0),
    "k_check_se2_paths_footprint": (0, 0),
    "k_check_rs_paths_footprint": (112, 0),
    "k_hybrid_search_footprint": (152, 4),
}


def test_footprint_kernel_resources():
    from pathplanning_amd import build
    import kernel_resources
    lib_path = build.build(verbose=False)
    res = {k["kernel"]: k for k in kernel_resources.resources(lib_path)}
    for name, (scratch, spills) in LIMITS.items():
        assert name in res, (name, sorted(res))
        k = res[name]
        assert k["scratch_bytes_per_lane"] <= scratch, (name, k)
        assert k["vgpr_spill"] <= spills, (name, k)
    assert res["k_check_rs_paths"]["scratch_bytes_per_lane"] == 112 and res["k_check_rs_paths"]["vgpr_spill"] == 0  # the counterpart the RS limit is taken from
    # the streamed form stages poses and flags through LDS like k_check_states_pipe (an LDS-resident bitmap form is not shipped)
    assert res["k_check_states_footprint_pipe"]["lds_bytes"] <= res["k_check_states_pipe"]["lds_bytes"] <= 160 * 1024
