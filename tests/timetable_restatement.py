"""A timetable call (include/pp_hip.h, "timetable look-ups and stops") restated in numpy, for tests/test_gpu_pipeline_timetable.py,
tests/test_timetable_restatement_host.py and tests/test_timetable_rule_host.py.  It shares nothing with the kernel: a profile is an [N, 3] array of
(s, v, t) rows as tests/speed_restatement.py (or the device) gives them, plans are the objects of tests/locate_restatement.py.  The forward direction
(time -> arc length), the pose and the step time are conflict_restatement's; the stops, the inverse (arc length -> time), speed and acceleration and
the next-stop search are written here from the definition.  Every numpy operation is one correctly rounded double operation, in the header's order,
so that everything taken from the rows is bit-exact against the device when it is fed the device's own rows.

A look-up is DECIDED (edge, ratio and direction can be compared) when its arc length is more than EPS from every junction S_e, e >= 2 (S_1 = 0 is exact
on either side), and no closer than speed_restatement.GUARD to a boundary between two Reeds-Shepp motions.  A cusp stop at the junction of two edges is undecided by
nature: it is where the direction changes."""
import numpy as np

import locate_restatement as R
import speed_restatement as SP
from conflict_restatement import poses_at, position, step_time

EPS = 1e-9
MAX_STOPS = 1 << 16
MAX_LOOKUPS = 1 << 26

PLAN_DTYPE = np.dtype([("status", np.int32), ("n_samples", np.int32), ("n_stops", np.int32), ("n_listed", np.int32), ("s_first", np.float64), ("s_last", np.float64),
                       ("duration", np.float64)])
STOP_DTYPE = np.dtype([("row", np.int32), ("reserved", np.int32), ("s", np.float64), ("t_arrive", np.float64), ("t_depart", np.float64)])
RESULT_DTYPE = np.dtype([("status", np.int32), ("row", np.int32), ("edge", np.int32), ("direction", np.int32), ("s", np.float64), ("t", np.float64), ("v", np.float64),
                         ("a", np.float64), ("ratio", np.float64), ("kappa", np.float64), ("pose", np.float64, 3), ("next_stop", np.int32), ("reserved", np.int32),
                         ("s_to_stop", np.float64), ("t_to_stop", np.float64), ("t_remaining", np.float64), ("reserved1", np.float64)])
assert PLAN_DTYPE.itemsize == 40 and STOP_DTYPE.itemsize == 32 and RESULT_DTYPE.itemsize == 128


def _rows(rows):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    return rows, rows[:, 0], rows[:, 1], rows[:, 2]


def stops(rows, a_acc, a_dec):
    """every stop of a profile, in row order, as STOP_DTYPE records"""
    rows, s_, v_, t_ = _rows(rows)
    j = np.flatnonzero(v_ == 0.0)
    out = np.zeros(len(j), dtype=STOP_DTYPE)
    before = np.maximum(j - 1, 0)
    arrive = t_[before] + step_time(s_[j] - s_[before], v_[before], v_[j], np.float64(a_acc), np.float64(a_dec))
    out["row"], out["s"], out["t_arrive"], out["t_depart"] = j, s_[j], np.where(j == 0, 0.0, arrive), t_[j]
    return out


def by_time(rows, u, a_acc, a_dec):
    """(status, row, s, t, v, a) of a profile at the times u [m] since its start"""
    rows, s_, v_, t_ = _rows(rows)
    N, u = len(rows), np.asarray(u, dtype=np.float64)
    a_acc, a_dec = np.float64(a_acc), np.float64(a_dec)
    status = np.where(u < 0.0, 1, np.where(u > t_[-1], 2, 0))
    t = np.where(u < 0.0, 0.0, np.where(u > t_[-1], t_[-1], u))
    _, s = position(rows, t, a_acc, a_dec)
    j = np.clip(np.searchsorted(t_, t, side="right") - 1, 0, N - 1)
    j1 = np.minimum(j + 1, N - 1)
    v0, v1, ds, delta = v_[j], v_[j1], s_[j1] - s_[j], t - t_[j]
    m = step_time(ds, v0, v1, a_acc, a_dec)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a_trap = (v1 - v0) / m
        ta = np.sqrt(2.0 * (ds * a_dec / (a_acc + a_dec)) / a_acc)
        rising = delta <= ta
        v = np.where(v0 + v1 > 0.0, v0 + a_trap * delta, np.where(rising, a_acc * delta, a_dec * (m - delta)))
        a = np.where(v0 + v1 > 0.0, a_trap, np.where(rising, a_acc, -a_dec))
    dwelling = delta >= m
    v, a = np.where(dwelling, v1, v), np.where(dwelling, 0.0, a)
    flat = (j == N - 1) | (ds == 0.0)
    v, a = np.where(flat, v0, v), np.where(flat, 0.0, a)
    return status, j, s, t, v, a


def by_length(rows, s, a_acc, a_dec):
    """(status, row, s, t, v, a) of a profile at the arc lengths s [m]"""
    rows, s_, v_, t_ = _rows(rows)
    N, s = len(rows), np.asarray(s, dtype=np.float64)
    a_acc, a_dec = np.float64(a_acc), np.float64(a_dec)
    status = np.where(s < s_[0], 1, np.where(s > s_[-1], 2, 0))
    s = np.where(s < s_[0], s_[0], np.where(s > s_[-1], s_[-1], s))
    j = np.clip(np.searchsorted(s_, s, side="right") - 1, 0, N - 1)  # the largest j with s_j <= s: behind equal arc lengths the last one
    j1 = np.minimum(j + 1, N - 1)
    v0, v1, ds, sigma = v_[j], v_[j1], s_[j1] - s_[j], s - s_[j]
    m = step_time(ds, v0, v1, a_acc, a_dec)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a_trap = (v1 - v0) / m
        w = v0 * v0 + (2.0 * a_trap) * sigma
        v_trap = np.sqrt(np.where(w > 0.0, w, 0.0))
        d_trap = (2.0 * sigma) / (v0 + v_trap)
        x = ds * a_dec / (a_acc + a_dec)
        d_up = np.sqrt(2.0 * sigma / a_acc)
        r = np.sqrt(2.0 * (ds - sigma) / a_dec)
        up = sigma <= x
        trap = v0 + v1 > 0.0
        delta = np.where(trap, d_trap, np.where(up, d_up, m - r))
        v = np.where(trap, v_trap, np.where(up, a_acc * d_up, a_dec * r))
        a = np.where(trap, a_trap, np.where(up, a_acc, -a_dec))
    at_row = sigma == 0.0
    delta, v = np.where(at_row, 0.0, delta), np.where(at_row, v0, v)
    delta = np.where(delta >= 0.0, delta, 0.0)
    delta = np.where(delta > m, m, delta)
    t = t_[j] + delta
    last = j == N - 1
    return status, j, s, np.where(last, t_[j], t), np.where(last, v0, v), np.where(last, 0.0, a)


def direction_kappa(plan, s):
    """(edge, ratio, direction, kappa, decided) of a plan at the arc lengths s: the mapping of conflict_restatement.poses_at, then the path object's own
    travel direction and |curvature| at the ratio"""
    s = np.asarray(s, dtype=np.float64)
    n = len(s)
    if not plan.edges:
        return np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n), np.ones(n, dtype=bool)
    e = np.maximum(np.searchsorted(plan.S, s, side="right"), 1)
    L, S = plan.L[e - 1], plan.S[e - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(L > 0.0, np.minimum((s - S) / L, 1.0), 0.0)
    direction, kappa, decided = np.zeros(n, dtype=np.int64), np.zeros(n), np.ones(n, dtype=bool)
    for k, E in enumerate(plan.edges, start=1):
        at = e == k
        if not at.any():
            continue
        if isinstance(E, R.ArcEdge):
            direction[at], kappa[at] = (-1 if E.backward else 1), abs(E.kappa)
        else:
            direction[at], kappa[at], margin = SP.rs_motion(E.record, E.L, ratio[at])
            decided[at] = margin > SP.GUARD
    if len(plan.S) > 1:  # (S_1 = 0 is the same double on either side and no edge lies before it: nothing to decide there; the junctions are S_2 ..)
        decided &= np.abs(s[:, None] - plan.S[None, 1:]).min(axis=1) > EPS
    return e, ratio, direction, kappa, decided


def mixed_values(rows, by, P, a_acc, a_dec, seed=0, stops_too=False):
    """P values to look up in a profile, for the tests: before and behind it, on rows (the first, the last and eight others that are no junction
    samples -- a junction is sampled twice, at equal arc lengths), with stops_too on the inner stops and (by time) inside their dwells -- where a
    vehicle changes direction, so that at the junction of two edges no restatement decides edge or direction -- and the rest anywhere inside; rows None: P values that are
    looked at by nobody"""
    rng = np.random.RandomState(seed)
    if rows is None or len(rows) == 0:
        return rng.uniform(0.0, 10.0, P)
    rows, s_, v_, t_ = _rows(rows)
    col = t_ if by == "time" else s_
    st = stops(rows, a_acc, a_dec)
    fixed = [col[0] - 0.3, col[-1] + 0.4, col[0], col[-1], np.nextafter(col[-1], np.inf), np.nextafter(col[0], -np.inf)]
    alone = np.flatnonzero((np.diff(s_)[1:] > 0.0) & (np.diff(s_)[:-1] > 0.0) & (v_[1:-1] > 0.0)) + 1  # rows inside an edge that move
    if len(alone):
        fixed += list(col[alone[rng.randint(0, len(alone), 8)]])
    if stops_too:
        inner = st[(st["row"] > 0) & (st["row"] < len(rows) - 1)]
        fixed += list(col[inner["row"]][:8])
        if by == "time":
            dwelt = inner[inner["t_arrive"] < inner["t_depart"]]
            fixed += list(dwelt["t_arrive"] + 0.37 * (dwelt["t_depart"] - dwelt["t_arrive"]))[:8] + list(dwelt["t_arrive"][:4])
    fixed = fixed[:P]
    free = rng.uniform(col[0], col[-1], P - len(fixed))
    if by == "time" and not stops_too:  # a time drawn inside a dwell stands on a cusp stop: drawn again (at most a few per plan)
        for _ in range(64):
            inside = ((free[:, None] >= st["t_arrive"][None, 1:-1]) & (free[:, None] <= st["t_depart"][None, 1:-1])).any(axis=1) if len(st) > 2 else np.zeros(len(free), dtype=bool)
            if not inside.any():
                break
            free[inside] = rng.uniform(col[0], col[-1], int(inside.sum()))
    return np.concatenate([fixed, free]).astype(np.float64)


def timetable(plan, rows, values, by, a_acc, a_dec, max_stops=16):
    """what a timetable call owes for one plan (plan None or rows None: its profile has a status other than 0): (plan record, listed stops, results
    [P], decided [P]); `by` is "length" or "time"; plan may be given as False to leave pose, edge, ratio, direction and kappa out (zeros)"""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    rec, out = np.zeros((), dtype=PLAN_DTYPE), np.zeros(len(values), dtype=RESULT_DTYPE)
    if plan is None or rows is None or len(rows) == 0:
        rec["status"], out["status"] = -1, -1
        return rec, np.zeros(0, dtype=STOP_DTYPE), out, np.ones(len(values), dtype=bool)
    rows, s_, v_, t_ = _rows(rows)
    every = stops(rows, a_acc, a_dec)
    listed = every[:max_stops]
    rec["n_samples"], rec["n_stops"], rec["n_listed"] = len(rows), len(every), len(listed)
    rec["s_first"], rec["s_last"], rec["duration"] = s_[0], s_[-1], t_[-1]
    status, j, s, t, v, a = (by_time if by == "time" else by_length)(rows, values, a_acc, a_dec)
    out["status"], out["row"], out["s"], out["t"], out["v"], out["a"] = status, j, s, t, v, a
    decided = np.ones(len(values), dtype=bool)
    if plan is not False and len(values):
        out["pose"], _ = poses_at(plan, s)
        out["edge"], out["ratio"], out["direction"], out["kappa"], decided = direction_kappa(plan, s)
    k = np.searchsorted(listed["row"], j, side="right")  # the first listed stop with row > j
    found = k < len(listed)
    out["next_stop"] = np.where(found, k, -1)
    if len(listed):
        k = np.minimum(k, len(listed) - 1)
        out["s_to_stop"] = np.where(found, listed["s"][k] - s, 0.0)
        out["t_to_stop"] = np.where(found, listed["t_arrive"][k] - t, 0.0)
    out["t_remaining"] = t_[-1] - t
    return rec, listed, out, decided
