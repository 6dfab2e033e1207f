"""CPU: the numpy restatement of a locate call (tests/locate_restatement.py), which tests/test_gpu_pipeline_locate.py compares the kernel with, run
alone on the ORACLE's plans of that file's queries -- synthetic_world(256, 14, 3), validator (1.0, 0.1), the 48 query pairs of RandomState(7) -- with
that file's vehicle poses (RandomState(SEED)).  Checked without a GPU: the share of undecided cases stays within the 2 % the GPU comparison allows
(expected about 1e-4 per case: two neighbouring lattice points tie within 1e-9 m^2 only when the true minimum lies within 1.6e-7 m of their midpoint);
the located point is no worse than any stage-1 sample and than a scan of the plan ten times finer than the lattice by more than the lattice allows;
a vehicle on the plan is found where it stands; the scene has what the GPU cases need (a Reeds-Shepp edge with a cusp, an edge of more than 64
samples at spacing 0.01)."""
import math

import numpy as np

import locate_restatement as R
import oracle_lib as O
from test_gpu_pipeline_stamp import N, RES, _queries, _world

SEED = 11
MAX_UNDECIDED = 0.02
WHEELBASE, RMIN = 2.6, 2.0


def oracle_plans():
    w = _world()
    starts, goals, seeds = _queries(w, N)
    h = O.Hybrid(w)
    plans = []
    for q in range(N):
        r = h.search(starts[q], goals[q], int(seeds[q]))
        if r["status"] != 0:
            plans.append(None)
            continue
        poses, edges = r["path_poses"], []
        for e in range(1, len(poses)):
            L = float(r["path_length"][e])
            if r["path_kind"][e] == 1:
                edges.append(R.ArcEdge(poses[e - 1], L, math.tan(r["path_steering"][e]) / WHEELBASE, r["path_direction"][e] == 1))
            else:
                rec = O.rs_connect(poses[e - 1], goals[q], RMIN)
                assert abs(rec["length"][0] - L) < 1e-9
                edges.append(R.RsEdge(rec, L, O.rs_path_interpolate))
        plans.append(R.Plan(poses[0], edges))
    return plans, starts, goals


PLANS = None


def scene():
    global PLANS
    if PLANS is None:
        plans, starts, goals = oracle_plans()
        rng = np.random.RandomState(SEED)
        vehicles = [R.vehicle_poses(plans[q], starts[q], goals[q], 128 * RES, rng) for q in range(N)]
        PLANS = (plans, starts, goals, vehicles)
    return PLANS


def test_the_share_of_undecided_cases_is_within_the_cap():
    plans, _, _, vehicles = scene()
    assert sum(p is not None for p in plans) >= 40
    for spacing, w in ((0.1, 0.0), (0.37, 0.0), (0.1, 2.0)):
        cases = [R.locate(plans[q], v, spacing, w) for q in range(N) for v in vehicles[q]]
        located = [c for c in cases if c["status"] == 0]
        undecided = sum(not c["decided"] for c in located)
        print("spacing %g, heading weight %g: %d cases, %d located, %d undecided" % (spacing, w, len(cases), len(located), undecided))
        assert len(located) >= 300 and undecided <= MAX_UNDECIDED * len(cases)


def test_the_located_point_is_the_least_of_a_finer_scan():
    """cost <= every stage-1 sample's; and against a scan at delta / 10 over the whole plan: not worse by more than a lattice point can be
    (half a step along a cost whose slope is at most 2 (distance + w^2 pi / rmin)), unless the scan's minimum is a second valley that stage 1 missed
    between two samples -- which at spacing 0.1 and vehicles within 0.5 m of the plan does not happen on this scene"""
    plans, _, _, vehicles = scene()
    spacing, checked = 0.1, 0
    for q in range(0, N, 3):
        plan = plans[q]
        if plan is None or not plan.edges:
            continue
        u = np.arange(0.0, plan.length, spacing / 320.0)
        e = np.searchsorted(plan.S, u, side="right")
        poses, _ = plan.at(e, np.where(plan.L[e - 1] > 0, np.minimum((u - plan.S[e - 1]) / np.where(plan.L[e - 1] > 0, plan.L[e - 1], 1.0), 1.0), 0.0))
        for v in vehicles[q][:6]:  # near the plan, and the exact start
            got = R.locate(plan, v, spacing)
            fine = R.cost(v, poses, 0.0)
            assert got["c"] <= R.cost(v, plan.samples(spacing)[3], 0.0).min()
            slack = 2.0 * (math.sqrt(fine.min()) + 1e-3) * (0.5 * spacing / 32.0) + (0.5 * spacing / 32.0) ** 2
            assert got["c"] <= fine.min() + slack, (q, v, got["c"], fine.min())
            assert abs(got["distance"] ** 2 - got["c"]) < 1e-12 and got["distance"] <= 0.5 + 1e-9 or v is vehicles[q][5]
            checked += 1
    assert checked >= 60


def test_a_vehicle_on_the_plan_is_found_where_it_stands():
    plans, starts, goals, _ = scene()
    for q in range(N):
        plan = plans[q]
        if plan is None or not plan.edges:
            continue
        at_start, at_goal = R.locate(plan, starts[q], 0.1), R.locate(plan, goals[q], 0.1)
        assert (at_start["edge"], at_start["s"], at_start["ratio"], at_start["distance"]) == (1, 0.0, 0.0, 0.0) and at_start["decided"]
        assert at_goal["edge"] == len(plan.edges) and abs(at_goal["s"] - plan.length) < 0.1 / 32 and at_goal["distance"] < 1e-6
        # a pose of the plan's middle, with the window that holds it and with one that does not
        mid = R.locate(plan, plan.at([1], [0.5])[0][0], 0.1, lo=0.0, hi=plan.L[0])
        assert mid["edge"] == 1 and abs(mid["ratio"] - 0.5) < 0.1 / 32 / plan.L[0] + 1e-12 and mid["distance"] < 0.1 / 32
        assert R.locate(plan, starts[q], 0.1, lo=plan.length + 1.0)["status"] == 1
        assert R.locate(plan, starts[q], 0.1, lo=0.45 * plan.length)["s"] >= 0.45 * plan.length
    assert R.locate(None, starts[0], 0.1)["status"] == -1


def cusp_of(plan):
    """(arc length, ratio) of the first direction change inside the last edge of `plan`, if that is a Reeds-Shepp edge with one"""
    if plan is None or not plan.edges or not isinstance(plan.edges[-1], R.RsEdge):
        return None
    ratio = np.linspace(0.0, 1.0, 2001)
    d = plan.edges[-1].at(ratio)[1]
    k = np.flatnonzero(d[1:] != d[:-1])
    return (plan.S[-1] + 0.5 * (ratio[k[0]] + ratio[k[0] + 1]) * plan.L[-1], 0.5 * (ratio[k[0]] + ratio[k[0] + 1])) if len(k) else None


def test_the_scene_has_what_the_gpu_cases_need():
    plans, _, _, _ = scene()
    assert sum(cusp_of(p) is not None for p in plans) >= 1
    assert any(p is not None and p.edges and R.steps(p.L.max(), 0.01) > 64 for p in plans)
