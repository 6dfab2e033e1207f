"""CPU: the numpy restatement of a speed-profile call (tests/speed_restatement.py), which tests/test_gpu_pipeline_speed_profile.py compares the kernel
with, run alone on the ORACLE's plans of that file's queries (the scene of tests/test_locate_restatement_host.py: synthetic_world(256, 14, 3),
validator (1.0, 0.1), the 48 query pairs of RandomState(7)).  Checked without a GPU:
 - the FEASIBILITY of every profile, a property that needs no restatement: e_{j+1} <= e_j + 2 a_acc ds and e_j <= e_{j+1} + 2 a_dec ds (+ 1e-9),
   v <= cap, v == 0 at every cusp stop and at both ends when v_start == v_end == 0, times that do not decrease -- without and with the clearance term
   (the point disc and the three-disc CAR3 of tests/footprint_ref.py), with windows and end speeds;
 - the envelope against a plain sequential forward-then-backward sweep over the same caps;
 - that the share of undecided samples stays within footprint_ref.MAX_LEFT_OUT, which the GPU comparison allows;
 - that the scene has what the GPU cases need: spacings that give N < 64, N == 64, N == 65 and N > 128, a plan with a reverse primitive (a junction
   cusp), a Reeds-Shepp edge that changes direction inside."""
import numpy as np

import footprint_ref as FR
import locate_restatement as R
import speed_restatement as V
from test_gpu_pipeline_stamp import _world
from test_locate_restatement_host import cusp_of, scene

LIMITS = [V.limits(), V.limits(spacing=0.37, a_acc=0.8, a_dec=3.0, a_lat=0.9, dwell=1.5, v_max_forward=8.0, v_max_reverse=1.0)]


def solved():
    return [(q, p) for q, p in enumerate(scene()[0]) if p is not None]


def sweep(s, w, lim):
    e = w.copy()
    for j in range(1, len(s)):
        e[j] = min(e[j], e[j - 1] + 2.0 * lim["a_acc"] * (s[j] - s[j - 1]))
    for j in range(len(s) - 2, -1, -1):
        e[j] = min(e[j], e[j + 1] + 2.0 * lim["a_dec"] * (s[j + 1] - s[j]))
    return e


def test_every_profile_is_feasible_and_equals_the_sweep():
    checked = cusps = 0
    for lim in LIMITS:
        for q, plan in solved():
            p = V.profile(plan, lim)
            assert p["status"] == 0 and p["length"] == plan.length and p["s_first"] == 0.0 and abs(p["s_last"] - plan.length) < 1e-9
            V.feasible(p, lim)
            assert p["v"][0] == 0.0 and p["v"][-1] == 0.0 and p["duration"] > 0.0 or not plan.edges
            ref = sweep(p["s"], p["w"], lim)
            assert np.abs(p["e"] - ref).max() <= 1e-12 * max(ref.max(), 1.0) + 4 * 2.3e-16 * (2.0 * max(lim["a_acc"], lim["a_dec"]) * plan.length + p["w"].max())
            assert abs(p["v_peak"] - np.sqrt(ref.max())) < 1e-9
            # the time is at least the length at the peak speed, plus the dwells
            assert p["duration"] >= plan.length / max(p["v_peak"], 1e-300) - 1e-9 + p["n_cusps"] * lim["dwell"] or not plan.edges
            checked += 1
            cusps += p["n_cusps"]
    assert checked >= 80 and cusps >= 2


def test_windows_and_end_speeds():
    lim = LIMITS[0]
    for q, plan in solved()[:12]:
        if not plan.edges:
            continue
        lo, hi = 0.3 * plan.length, 0.8 * plan.length
        p = V.profile(plan, lim, lo, hi, 3.0, 1.5)
        V.feasible(p, lim, 3.0, 1.5)
        assert lo <= p["s_first"] <= lo + lim["spacing"] and hi - lim["spacing"] <= p["s_last"] <= hi
        assert p["v"][0] == min(p["cap"][0], 3.0) or p["cusp"][0] or p["v"][0] < 3.0
        assert V.profile(plan, lim, plan.length + 1.0)["status"] == 1
        assert V.profile(plan, lim, max_samples=p["n_samples"])["status"] == -5
    assert V.profile(None, lim)["status"] == -1


def test_the_clearance_term_lowers_speeds_and_stays_decided():
    w = _world()
    grid = FR.Grid(w)
    samples = undecided = 0
    for discs in ([(0.0, 0.0, 1.0)], FR.CAR3):
        lim = V.limits(clearance_gain=1.5, v_floor=0.3)
        for q, plan in solved():
            free, p = V.profile(plan, V.limits()), V.profile(plan, lim, clearance=V.grid_clearance(grid, discs))
            V.feasible(p, lim)
            assert (p["v"] <= free["v"] + 1e-12).all() and p["min_clearance"] == float(p["cl"].min()) and p["min_clearance"] >= 0.0
            assert p["s_min_clearance"] == p["s"][int(np.argmin(p["cl"]))]
            assert (p["cap"] <= 0.3 + 1.5 * p["cl"].astype(np.float64)).all()
            samples += p["n_samples"]
            undecided += int((~p["decided"]).sum())
    print("%d samples, %d undecided" % (samples, undecided))
    assert samples > 10000 and undecided <= FR.MAX_LEFT_OUT * samples


def test_the_scene_has_what_the_gpu_cases_need():
    plans = [p for _, p in solved()]
    for target in (64, 65):
        assert V.find_spacing(plans, lambda n: n == target) is not None, target
    assert V.find_spacing(plans, lambda n: 8 < n < 64) is not None and V.find_spacing(plans, lambda n: n > 128) is not None
    assert any(p.edges and any(isinstance(E, R.ArcEdge) and E.backward for E in p.edges) and V.profile(p, LIMITS[0])["n_cusps"] >= 1 for p in plans)
    inside = [p for p in plans if cusp_of(p) is not None]
    assert inside and all(V.profile(p, LIMITS[0])["n_cusps"] >= 1 for p in inside)
    # the stop of a direction change inside the Reeds-Shepp edge lies at the first sample behind it, at most `spacing` late
    for p in inside:
        sc, _ = cusp_of(p)
        prof = V.profile(p, LIMITS[0])
        stops = prof["s"][prof["cusp"]]
        assert ((stops >= sc - 1e-3) & (stops <= sc + 0.1 + 1e-3)).any(), (sc, stops)
