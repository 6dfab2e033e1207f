"""A conflict call (include/pp_hip.h, "space-time conflicts between held plans") restated in numpy, for tests/test_gpu_pipeline_conflicts.py,
tests/test_conflict_restatement_host.py and tests/test_conflict_rule_host.py.  It shares nothing with the kernels: plans and edges are the objects of
tests/locate_restatement.py, a profile is an [N, 3] array of (s, v, t) rows as tests/speed_restatement.py (or the device) gives them; the lattice, the
row search, the position within a step, the disc centres, the separation and the two orders are written here from the definition.  Every numpy
operation is one correctly rounded double operation, in the header's order, so that the row search and s(u) are bit-exact against the device when it
is fed the device's own rows.

A pair-time is UNDECIDED when |separation - margin| <= EPS = 1e-9 (device and glibc poses differ around 1e-12 m) or one of its two poses is undecided;
a pose is undecided under speed_restatement's Reeds-Shepp boundary rule (closer than GUARD to a boundary between two motions)."""
import math

import numpy as np

import locate_restatement as R
import speed_restatement as SP

EPS = 1e-9
MAX_TIMES = 1 << 20


def lattice(t_from, t_to, dt):
    """(k0, T): k0 = ceil(t_from / dt) and k1 = floor(t_to / dt), clipped to +-2^62 in double before the conversion; T = k1 - k0 + 1 (0: none)"""
    def index(q):
        q = np.float64(q)
        if not q < 2.0 ** 62:
            q = 2.0 ** 62
        if q < -2.0 ** 62:
            q = -2.0 ** 62
        return int(q)
    with np.errstate(over="ignore"):
        k0, k1 = index(np.ceil(np.float64(t_from) / np.float64(dt))), index(np.floor(np.float64(t_to) / np.float64(dt)))
    return k0, max(k1 - k0 + 1, 0)


def times(k0, T, dt):
    """tau_m = (double)(k0 + m) * dt"""
    return np.array([float(k0 + m) for m in range(T)], dtype=np.float64) * np.float64(dt)


def step_time(ds, v0, v1, a_acc, a_dec):
    """the motion time of a step (speed profiles, "Time"), elementwise"""
    with np.errstate(divide="ignore", invalid="ignore"):
        x = ds * a_dec / (a_acc + a_dec)
        triangle = np.sqrt(2.0 * x / a_acc) + np.sqrt(2.0 * (ds - x) / a_dec)
        return np.where(ds == 0.0, 0.0, np.where(v0 + v1 > 0.0, (2.0 * ds) / (v0 + v1), triangle))


def position(rows, u, a_acc, a_dec, hold_before=False, hold_after=False):
    """(present [m] bool, s [m]) of a vehicle with the profile rows [N, 3] at the times u [m] after its start"""
    rows, u = np.asarray(rows, dtype=np.float64).reshape(-1, 3), np.asarray(u, dtype=np.float64)
    s_, v_, t_ = rows[:, 0], rows[:, 1], rows[:, 2]
    N = len(rows)
    a_acc, a_dec = np.float64(a_acc), np.float64(a_dec)
    before, after = u < 0.0, u > t_[-1]
    j = np.clip(np.searchsorted(t_, u, side="right") - 1, 0, N - 1)  # the largest j with t_j <= u: behind equal times the last one
    j1 = np.minimum(j + 1, N - 1)
    s0, v0, s1, v1 = s_[j], v_[j], s_[j1], v_[j1]
    ds, delta = s1 - s0, u - t_[j]
    m = step_time(ds, v0, v1, a_acc, a_dec)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = (v1 - v0) / m
        trapezoid = s0 + (v0 + (0.5 * a) * delta) * delta
        x = ds * a_dec / (a_acc + a_dec)
        ta = np.sqrt(2.0 * x / a_acc)
        r = m - delta
        triangle = np.where(delta <= ta, s0 + (0.5 * a_acc) * delta * delta, s1 - (0.5 * a_dec) * r * r)
        s = np.where(v0 + v1 > 0.0, trapezoid, triangle)
    s = np.where(s < s0, s0, s)
    s = np.where(s > s1, s1, s)
    s = np.where(delta >= m, s1, s)
    s = np.where((j == N - 1) | (ds == 0.0), s0, s)
    s = np.where(before, s_[0], np.where(after, s_[-1], s))
    present = np.where(before, bool(hold_before), np.where(after, bool(hold_after), True))
    return present, s


def poses_at(plan, s):
    """(poses [m, 3], decided [m]) of a plan at the arc lengths s: the locate call's lattice mapping, then the edge's interpolation"""
    s = np.asarray(s, dtype=np.float64)
    if not plan.edges:
        return np.repeat(plan.first[None], len(s), axis=0), np.ones(len(s), dtype=bool)
    if len(s) == 0:
        return np.empty((0, 3)), np.ones(0, dtype=bool)
    e = np.maximum(np.searchsorted(plan.S, s, side="right"), 1)  # the largest e with S_e <= s
    L, S = plan.L[e - 1], plan.S[e - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(L > 0.0, np.minimum((s - S) / L, 1.0), 0.0)
    poses, _ = plan.at(e, ratio)
    decided = np.ones(len(s), dtype=bool)
    for k, E in enumerate(plan.edges, start=1):
        if isinstance(E, R.RsEdge) and (e == k).any():
            decided[e == k] = SP.rs_motion(E.record, E.L, ratio[e == k])[2] > SP.GUARD
    return poses, decided


def trajectory(plan, rows, t_start, tau, a_acc, a_dec, hold_before=False, hold_after=False):
    """what a conflict call owes for one plan (None, or rows None: its profile has a status other than 0): the record's fields and, for status >= 0,
    the arrays present, s, poses (NaN where absent) and decided over the lattice"""
    T = len(tau)
    none = dict(n_present=0, first=-1, last=-1, s_enter=0.0, s_leave=0.0)
    if plan is None or rows is None or len(rows) == 0:
        return dict(none, status=-1, present=np.zeros(T, dtype=bool), poses=np.full((T, 3), np.nan))
    present, s = position(rows, tau - np.float64(t_start), a_acc, a_dec, hold_before, hold_after)
    poses, decided = np.full((T, 3), np.nan), np.ones(T, dtype=bool)
    poses[present], decided[present] = poses_at(plan, s[present])
    k = np.flatnonzero(present)
    rec = dict(none, status=1) if len(k) == 0 else dict(status=0, n_present=len(k), first=int(k[0]), last=int(k[-1]), s_enter=float(s[k[0]]), s_leave=float(s[k[-1]]))
    return dict(rec, present=present, s=s, poses=poses, decided=decided)


def centres(poses, discs):
    """[K, m, 2]: the discs' centres in the world ("vehicle footprint": the parentheses are part of the definition)"""
    x, y, t = poses[:, 0], poses[:, 1], poses[:, 2]
    out = []
    for ox, oy, _ in discs:
        out.append((x, y) if ox == 0.0 and oy == 0.0 else ((x + ox * np.cos(t)) - oy * np.sin(t), (y + ox * np.sin(t)) + oy * np.cos(t)))
    return np.array(out).transpose(0, 2, 1).reshape(len(discs), len(x), 2)


def pair(A, B, tau, discs, margin):
    """the pair record of two trajectories (trajectory()'s dicts) over the lattice tau, with `separation` [n_times] at the times `both`, and `undecided`:
    how many of those times are"""
    zero = dict(n_times=0, n_conflict=0, t_first=0.0, s_first=(0.0, 0.0), min_separation=0.0, t_min=0.0, s_min=(0.0, 0.0), undecided=0,
                both=np.zeros(0, dtype=np.int64), separation=np.zeros(0))
    if A["status"] < 0 or B["status"] < 0:
        return dict(zero, status=-1)
    both = np.flatnonzero(A["present"] & B["present"])
    if len(both) == 0:
        return dict(zero, status=2, min_separation=math.inf)
    ca, cb = centres(A["poses"][both], discs), centres(B["poses"][both], discs)
    radius = np.array([np.float64(np.float32(r)) for _, _, r in discs])
    sep = np.full(len(both), np.inf)
    for i in range(len(discs)):
        for j in range(len(discs)):
            dx, dy = ca[i, :, 0] - cb[j, :, 0], ca[i, :, 1] - cb[j, :, 1]
            sep = np.minimum(sep, np.sqrt(dx * dx + dy * dy) - (radius[i] + radius[j]))
    conflict = sep < np.float64(margin)
    undecided = (np.abs(sep - np.float64(margin)) <= EPS) | ~A["decided"][both] | ~B["decided"][both]
    k = int(np.argmin(sep))  # (the first of equals: the smallest tau)
    rec = dict(status=1 if conflict.any() else 0, n_times=len(both), n_conflict=int(conflict.sum()), t_first=0.0, s_first=(0.0, 0.0), min_separation=float(sep[k]),
               t_min=float(tau[both[k]]), s_min=(float(A["s"][both[k]]), float(B["s"][both[k]])), undecided=int(undecided.sum()), both=both, separation=sep,
               conflict=conflict, undecided_at=undecided)
    if conflict.any():
        f = both[int(np.argmax(conflict))]
        rec.update(t_first=float(tau[f]), s_first=(float(A["s"][f]), float(B["s"][f])))
    return rec


def all_pairs(n):
    """every i < j, row-major"""
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def conflicts(plans, rows, t_start, pairs, discs, a_acc, a_dec, t_from, t_to, dt, margin=0.0, hold_before=False, hold_after=False):
    """(tau, trajectories, pair records) of a whole call; pairs None: every i < j"""
    k0, T = lattice(t_from, t_to, dt)
    assert 1 <= T <= MAX_TIMES
    tau = times(k0, T, dt)
    traj = [trajectory(p, r, t0, tau, a_acc, a_dec, hold_before, hold_after) for p, r, t0 in zip(plans, rows, t_start)]
    pairs = all_pairs(len(plans)) if pairs is None else pairs
    return tau, traj, [pair(traj[a], traj[b], tau, discs, margin) for a, b in pairs]
