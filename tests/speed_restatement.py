"""A speed-profile call (include/pp_hip.h, "speed profiles along held plans") restated in numpy, for tests/test_gpu_pipeline_speed_profile.py and
tests/test_speed_restatement_host.py.  It shares nothing with the kernel: plans and edges are the objects of tests/locate_restatement.py (which also
gives the schedule); the direction and curvature of a Reeds-Shepp sample are read from the record by GetDirection's selection written out here; the
carried direction, the cusp flag, the cap, the two envelopes and the times are written from the definition.  np.minimum.accumulate is the exact
running minimum, np.sqrt is correctly rounded, and t is the sequential sum.

A sample is DECIDED when its Reeds-Shepp sample lies more than GUARD = 1e-9 m from a boundary between two motions and, with a clearance term, every
disc centre (and the reference point) lies more than GUARD from a cell border of the target: only there can poses that differ around 1e-12 m
(device against glibc) choose another cap."""
import math

import numpy as np

import footprint_ref as FR
import locate_restatement as R

GUARD = 1e-9
DEFAULTS = dict(spacing=0.1, v_max_forward=5.0, v_max_reverse=2.0, a_acc=1.5, a_dec=2.5, a_lat=2.0, dwell=0.0, clearance_gain=0.0, v_floor=0.0)


def limits(**kw):
    assert not set(kw) - set(DEFAULTS)
    return dict(DEFAULTS, **kw)


def rs_motion(rec, L, ratio):
    """PathReedsShepp::GetDirection's selection on a record (one element of RS_PATH_DTYPE) of length L: per ratio the travel direction (+1 / -1; 0: no
    motion), kappa (1 / rmin on a turn, 0 on a straight) and the distance in metres to the nearest boundary between two motions"""
    rec = np.asarray(rec).reshape(-1)[0]
    rmin = float(rec["min_turning_radius"])
    target = np.asarray(ratio, dtype=np.float64) * np.float64(L)
    direction, kappa = np.zeros(len(target), dtype=np.int64), np.zeros(len(target))
    margin, chosen = np.full(len(target), np.inf), np.zeros(len(target), dtype=bool)
    if L == 0:
        return direction, kappa, margin
    valid = []
    for i in range(5):  # (the loop stops at the first invalid motion)
        if not np.isfinite(rec["motion_length"][i]) or rec["direction"][i] == 2:
            break
        valid.append(i)
    length = np.float64(0.0)
    for i in valid:
        length = length + np.float64(rec["motion_length"][i]) * np.float64(rmin)
        if i != valid[-1]:
            margin = np.minimum(margin, np.abs(target - length))
        take = ~chosen & (target <= length)
        direction[take] = -1 if rec["direction"][i] == 1 else 1
        kappa[take] = 0.0 if rec["steer"][i] == 1 else 1.0 / rmin
        chosen |= take
    return direction, kappa, margin


def schedule(plan, spacing):
    """(s, poses, own direction, kappa, margin to a motion boundary) of every sample of the stamp's schedule"""
    if not plan.edges:
        return np.zeros(1), plan.first[None].copy(), np.zeros(1, dtype=np.int64), np.zeros(1), np.full(1, np.inf)
    edge, ratio, arc, poses, _ = plan.samples(spacing)
    direction, kappa, margin = np.zeros(len(arc), dtype=np.int64), np.zeros(len(arc)), np.full(len(arc), np.inf)
    for e, E in enumerate(plan.edges, start=1):
        k = edge == e
        if isinstance(E, R.ArcEdge):
            direction[k], kappa[k] = (-1 if E.backward else 1), abs(E.kappa)
        else:
            direction[k], kappa[k], margin[k] = rs_motion(E.record, E.L, ratio[k])
    return arc, poses, direction, kappa, margin


def grid_clearance(grid, discs):
    """poses -> (cl_j as float32, near a cell border) on a footprint_ref.Grid, by footprint_ref.fp_state"""
    def clearance(poses):
        ok, clear, _, _ = FR.fp_state(grid, poses, discs)
        x, y, t = poses[:, 0], poses[:, 1], poses[:, 2]
        near = np.zeros(len(poses), dtype=bool)
        for ox, oy, _ in [(0.0, 0.0, 0.0)] + list(discs):
            cx, cy = (x, y) if ox == 0 and oy == 0 else ((x + ox * np.cos(t)) - oy * np.sin(t), (y + ox * np.sin(t)) + oy * np.cos(t))
            _, _, qx, qy = FR.cell(grid, cx, cy)
            near |= (np.abs(qx - np.rint(qx)) * grid.resd < GUARD) | (np.abs(qy - np.rint(qy)) * grid.resd < GUARD)
        return np.where(ok, clear, FR.F32(0)).astype(FR.F32), near
    return clearance


def envelope_and_times(s, cap, cusp, lim, v_start, v_end):
    """(w, e, v, t) of a sequence from its arc lengths, caps and cusp flags"""
    n = len(s)
    w = cap * cap
    w[cusp] = 0.0
    w[0] = min(w[0], v_start * v_start)
    w[-1] = min(w[-1], v_end * v_end)
    ka, kd = 2.0 * lim["a_acc"], 2.0 * lim["a_dec"]
    fwd = np.minimum.accumulate(w - ka * s) + ka * s
    bwd = np.minimum.accumulate((w + kd * s)[::-1])[::-1] - kd * s
    m = np.minimum(w, np.minimum(fwd, bwd))
    e = np.where(m > 0.0, m, 0.0)
    v = np.sqrt(e)
    t = np.zeros(n)
    for j in range(n - 1):  # the sequential sum
        ds, both = s[j + 1] - s[j], v[j] + v[j + 1]
        if ds == 0.0:
            dt = 0.0
        elif both > 0.0:
            dt = (2.0 * ds) / both
        else:
            x = ds * lim["a_dec"] / (lim["a_acc"] + lim["a_dec"])
            dt = math.sqrt(2.0 * x / lim["a_acc"]) + math.sqrt(2.0 * (ds - x) / lim["a_dec"])
        t[j + 1] = t[j] + (dt + (lim["dwell"] if cusp[j + 1] else 0.0))
    return w, e, v, t


def profile(plan, lim, lo=-np.inf, hi=np.inf, v_start=0.0, v_end=0.0, max_samples=1 << 30, clearance=None):
    """what a speed-profile call owes for `plan` (None: no plan): the record's fields and, for status 0, the arrays s, v, t, cap, cusp, e, decided"""
    zero = dict(n_cusps=0, s_first=0.0, s_last=0.0, duration=0.0, v_peak=0.0, min_clearance=0.0, s_min_clearance=0.0)
    if plan is None:
        return dict(zero, status=-1, n_samples=0, length=0.0)
    arc, poses, own, kappa, margin = schedule(plan, lim["spacing"])
    keep = np.flatnonzero((arc >= lo) & (arc <= hi))
    n = len(keep)
    if n == 0 or n > max_samples:
        return dict(zero, status=1 if n == 0 else -5, n_samples=n, length=plan.length)
    assert np.array_equal(keep, np.arange(keep[0], keep[0] + n))  # one run of the schedule
    s, poses, own, kappa, decided = arc[keep], poses[keep], own[keep], kappa[keep], margin[keep] > GUARD
    # the direction a sample counts with: its own, or the one of the last sample before it that moves
    last = np.maximum.accumulate(np.where(own != 0, np.arange(n), -1))
    direction = np.where(last >= 0, own[np.maximum(last, 0)], 0)
    previous = np.concatenate([[0], direction[:-1]])
    cusp = (direction != 0) & (previous != 0) & (direction != previous)
    cap = np.where(direction == 1, np.float64(lim["v_max_forward"]), np.float64(lim["v_max_reverse"]))
    with np.errstate(divide="ignore"):
        cap = np.where(kappa > 0.0, np.minimum(cap, np.sqrt(np.float64(lim["a_lat"]) / np.where(kappa > 0.0, kappa, 1.0))), cap)
    cl = None
    if lim["clearance_gain"] > 0.0:
        cl, near = clearance(poses)
        decided &= ~near
        cap = np.minimum(cap, np.float64(lim["v_floor"]) + np.float64(lim["clearance_gain"]) * cl.astype(np.float64))
    w, e, v, t = envelope_and_times(s, cap, cusp, lim, v_start, v_end)
    k = int(np.argmin(cl)) if cl is not None else 0  # (the first of equals: the smallest s)
    return dict(status=0, n_samples=n, n_cusps=int(cusp.sum()), length=plan.length, s_first=float(s[0]), s_last=float(s[-1]), duration=float(t[-1]), v_peak=float(v.max()),
                min_clearance=float(cl[k]) if cl is not None else math.inf, s_min_clearance=float(s[k]) if cl is not None else 0.0,
                s=s, v=v, t=t, cap=cap, cusp=cusp, e=e, w=w, decided=decided, poses=poses, direction=direction, cl=cl)


def feasible(p, lim, v_start=0.0, v_end=0.0, tol=1e-9):
    """the property a profile must have whatever computed it: no step accelerates beyond a_acc or brakes beyond a_dec, no speed exceeds its cap, the
    vehicle stands at every cusp stop, and starts and ends no faster than asked"""
    s, e, v = p["s"], p["e"], p["v"]
    ds = s[1:] - s[:-1]
    assert (ds >= 0.0).all()
    assert (e[1:] <= e[:-1] + 2.0 * lim["a_acc"] * ds + tol).all()
    assert (e[:-1] <= e[1:] + 2.0 * lim["a_dec"] * ds + tol).all()
    assert (v <= p["cap"] * (1.0 + 1e-15)).all() and (v >= 0.0).all()
    assert (v[p["cusp"]] == 0.0).all()
    assert v[0] <= v_start and v[-1] <= v_end
    assert (p["t"][1:] >= p["t"][:-1]).all() and p["t"][0] == 0.0


def count(plan, spacing):
    """samples of the whole plan"""
    return sum(R.steps(L, spacing) + 1 for L in plan.L) if plan.edges else 1


def find_spacing(plans, wanted, spacings=None):
    """(index, spacing, N) of the first plan and spacing (2.000, 1.995, ... 0.050 m) whose whole-plan sample count satisfies `wanted`; None: there is none"""
    spacings = [round(2.0 - 0.005 * k, 3) for k in range(391)] if spacings is None else spacings
    for q, plan in enumerate(plans):
        if plan is None or not plan.edges:
            continue
        for spacing in spacings:
            if wanted(count(plan, spacing)):
                return q, spacing, count(plan, spacing)
    return None
