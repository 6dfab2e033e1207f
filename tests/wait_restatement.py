"""A call with waits at stops (include/pp_hip.h, "waits at stops that clear conflicts") restated in numpy on top of tests/conflict_restatement.py,
tests/delay_restatement.py and tests/timetable_restatement.py, for tests/test_gpu_pipeline_deconflict_waits.py, tests/test_wait_restatement_host.py and
tests/test_wait_rule_host.py.  It shares nothing with the kernels or with pp_wait_rule.hpp: the extended trajectory is conflict_restatement.trajectory
over the lattice indices k0 - D .. k1, the stops are timetable_restatement.stops, the arrive column is a linear scan, a vehicle under a wait is a
COMPOSITE trajectory gathered from the extended one and the standing pose, and every candidate is evaluated -- the shortcut the header permits is not
taken here, so the comparison checks it.

UNDECIDED is delay_restatement's notion: a vehicle is undecided when a separation of a candidate it tried lies within EPS = 1e-9 of the margin, and so
is every vehicle below it that is reachable through pairs."""
import numpy as np

import conflict_restatement as CR
import delay_restatement as DR
import timetable_restatement as TT

EPS = CR.EPS
FREE, NO_WAIT, START = -2, -2, -1
MAX_PLACES = 1 << 10

RESULT_DTYPE = np.dtype([("status", np.int32), ("place", np.int32), ("row", np.int32), ("wait_steps", np.int32), ("n_tried", np.int32), ("blocker", np.int32),
                         ("t_start", np.float64), ("t_hold", np.float64), ("t_resume", np.float64), ("s_wait", np.float64), ("t_block", np.float64), ("s_block", np.float64, 2)])
PLACE_DTYPE = np.dtype([("row", np.int32), ("column", np.int32), ("s", np.float64), ("t_arrive", np.float64), ("pose", np.float64, 3), ("sin_theta", np.float64),
                        ("cos_theta", np.float64)])
assert RESULT_DTYPE.itemsize == 80 and PLACE_DTYPE.itemsize == 64


def arrive_column(kE, columns, dt, t_start, t_arrive):
    """the smallest c in 0 .. columns - 1 with u_c = (double)(kE + c) * dt - t_start >= t_arrive, or `columns`"""
    u = CR.times(kE, columns, dt) - np.float64(t_start)
    at = np.flatnonzero(u >= np.float64(t_arrive))
    return int(at[0]) if len(at) else int(columns)


def source(c, a, d):
    """the column a vehicle that waits d steps at the stop with arrive column a reads at column c, or -1: it stands at the stop"""
    if d == 0 or c < a:
        return c
    return -1 if c < a + d else c - d


def candidates(D, start, P):
    """the candidates of a free vehicle in the order they are tried: (place, d)"""
    out = [(NO_WAIT, 0)]
    for d in range(1, D + 1):
        if start:
            out.append((START, d))
        out += [(q, d) for q in range(P)]
    return out


def stop_places(plan, rows, t_start, kE, columns, dt, a_acc, a_dec):
    """every stop of a profile as a place: PLACE_DTYPE records in row order, whatever their arrive column"""
    st = TT.stops(rows, a_acc, a_dec)
    out = np.zeros(len(st), dtype=PLACE_DTYPE)
    out["row"], out["s"], out["t_arrive"] = st["row"], st["s"], st["t_arrive"]
    out["column"] = [arrive_column(kE, columns, dt, t_start, t) for t in st["t_arrive"]]
    if len(st):
        out["pose"], _ = CR.poses_at(plan, st["s"])
        out["sin_theta"], out["cos_theta"] = np.sin(out["pose"][:, 2]), np.cos(out["pose"][:, 2])
    return out


def places_of(every, N, D, columns, max_places, fixed_row=FREE):
    """(listed places, qualifies) of a vehicle from all its stops: a free vehicle's first max_places inner stops reached inside the horizon; a fixed
    vehicle's one row (qualifies False: it is no stop reached before the horizon ends); a start wait lists nothing"""
    if fixed_row == START:
        return every[:0], True
    if fixed_row >= 0:
        mine = every[(every["row"] == fixed_row) & (every["column"] < columns)]
        return mine, len(mine) == 1
    inner = every[(every["row"] > 0) & (every["row"] < N - 1) & (every["column"] >= D) & (every["column"] < columns)]
    return inner[:max_places], True


def composite(t, place, d, T, D, spot=None):
    """conflict_restatement.trajectory's dict of a vehicle under the wait (place, d) over the T lattice times, from its extended trajectory t; spot is
    the PLACE_DTYPE record of a stop (place >= 0)"""
    c = np.arange(T) + D
    if place == START:
        src = c - d
    elif place >= 0 and d > 0:
        src = np.array([source(int(x), int(spot["column"]), d) for x in c])
    else:
        src = c
    standing = src < 0
    at = np.where(standing, 0, src)
    out = dict(status=t["status"], present=t["present"][at] | standing, poses=t["poses"][at].copy(), s=t["s"][at].copy(), decided=t["decided"][at].copy(), standing=standing)
    if standing.any():
        out["poses"][standing], out["s"][standing], out["decided"][standing] = spot["pose"], spot["s"], True
    return out


def least_key(mine, theirs, below, n, discs, radius, margin):
    """(the least key (m, j) of a composite against the composites of its scheduled partners, or None; whether a separation is undecided)"""
    best, undecided = None, False
    ca = None
    for j in sorted(set(below)):
        if theirs[j] is None:
            continue
        both = np.flatnonzero(mine["present"] & theirs[j]["present"])
        if not len(both):
            continue
        if ca is None:
            ca = CR.centres(np.nan_to_num(mine["poses"]), discs)
        sep = DR.separations(ca[:, both], theirs[j]["centres"][:, both], radius)
        undecided |= bool((np.abs(sep - margin) <= EPS).any())
        hit = np.flatnonzero(sep < margin)
        if len(hit):
            k = DR.key(int(both[hit[0]]), n, j)
            best = k if best is None or k < best else best
    return best, undecided


def decide(traj, every, tau, k0, T, D, n, pairs, discs, margin, t_start, dt, max_places, no_start_wait, fixed, listed=None):
    """the records of a call from the extended trajectories and every vehicle's stops (stop_places); listed (per vehicle a PLACE_DTYPE array, or None
    for a fixed row that does not qualify): the places are taken from there, not chosen here"""
    below = DR.partners_below(n, pairs)
    radius = np.array([np.float64(np.float32(r)) for _, _, r in discs])
    margin, dt = np.float64(margin), np.float64(dt)
    columns = T + D
    recs = np.zeros(n, dtype=RESULT_DTYPE)
    recs["place"], recs["row"], recs["wait_steps"], recs["blocker"] = NO_WAIT, -1, -1, -1
    undecided, theirs, chosen, spots = [False] * n, [None] * n, [None] * n, [None] * n
    for i in range(n):
        rec = recs[i]
        if traj[i]["status"] < 0:
            rec["status"] = -1
            continue
        fx = (FREE, 0) if fixed is None else (int(fixed[i][0]), int(fixed[i][1]))
        N = traj[i]["N"]
        if listed is not None:
            mine, ok = (listed[i], True) if listed[i] is not None else (None, False)
        else:
            mine, ok = places_of(every[i], N, D, columns, max_places, fx[0])
        if not ok:
            rec["status"] = -2
            continue
        spots[i] = mine
        undecided[i] = any(undecided[j] for j in below[i])
        if fx[0] == FREE:
            tried = candidates(D, not (no_start_wait is not None and no_start_wait[i]), len(mine))
        else:
            tried = [((START if fx[0] == START else 0) if fx[1] > 0 else NO_WAIT, fx[1])]
        blocked = None
        for o, (place, d) in enumerate(tried):
            comp = composite(traj[i], place, d, T, D, mine[place] if place >= 0 else None)
            best, close = least_key(comp, theirs, below[i], n, discs, radius, margin)
            undecided[i] |= close
            rec["n_tried"] = o + 1
            if best is None or fx[0] != FREE:
                chosen[i] = (place, d, comp)
            if best is None:
                break
            blocked = (best // n, best % n, comp)
        rec["t_start"] = t_start[i]
        if chosen[i] is None:
            rec["status"] = 1
        else:
            place, d, comp = chosen[i]
            rec["status"] = 2 if fx[0] != FREE and blocked is not None else 0
            rec["wait_steps"] = d
            comp["centres"] = CR.centres(np.nan_to_num(comp["poses"]), discs)
            theirs[i] = comp
            if place < 0:  # (no wait, or the start: the delay call's expression, also for d = 0 -- a start of -0.0 becomes 0.0)
                rec["place"] = place
                rec["t_start"] = np.float64(t_start[i]) + np.float64(d) * dt
            else:
                a = int(mine[place]["column"])
                rec["place"], rec["row"], rec["s_wait"] = place, mine[place]["row"], mine[place]["s"]
                rec["t_hold"], rec["t_resume"] = np.float64(float(k0 - D + a)) * dt, np.float64(float(k0 - D + a + d)) * dt
        if blocked is not None:
            m, j, comp = blocked
            rec["blocker"], rec["t_block"], rec["s_block"] = j, tau[m], (comp["s"][m], theirs[j]["s"][m])
    return recs, np.array(undecided), theirs, spots


def deconflict_waits(plans, rows, t_start, pairs, discs, a_acc, a_dec, t_from, t_to, dt, margin=0.0, hold_before=False, hold_after=False, max_delay_steps=0, max_places=0,
                     no_start_wait=None, fixed=None, poses=None, listed=None):
    """(tau, extended trajectories, records, undecided [n], composites of the scheduled vehicles, listed places per vehicle) of a whole call; pairs None:
    every pair.  poses (a list of [T + D, 3] arrays, NaN where absent) and listed (per vehicle the device's places, None for status -2): the bit-exact
    mode of the GPU test, in which the extended trajectories' poses and the places are the device's own, not restated"""
    k0, T = CR.lattice(t_from, t_to, dt)
    D = int(max_delay_steps)
    assert 1 <= T and D >= 0 and T + D <= CR.MAX_TIMES and 0 <= max_places <= MAX_PLACES
    n = len(plans)
    tau, extended = CR.times(k0, T, dt), CR.times(k0 - D, T + D, dt)
    traj = [CR.trajectory(p, r, t0, extended, a_acc, a_dec, hold_before, hold_after) for p, r, t0 in zip(plans, rows, t_start)]
    if poses is not None:
        for t, xyt in zip(traj, poses):
            if t["status"] >= 0:
                t["poses"], t["present"] = np.asarray(xyt, dtype=np.float64), ~np.isnan(np.asarray(xyt)[:, 0])
    every = [None] * n
    for i, (p, r, t0) in enumerate(zip(plans, rows, t_start)):
        if traj[i]["status"] >= 0:
            traj[i]["N"] = len(r)
            every[i] = stop_places(p, r, t0, k0 - D, T + D, dt, a_acc, a_dec) if listed is None else None
    recs, undecided, theirs, spots = decide(traj, every, tau, k0, T, D, n, pairs, discs, margin, t_start, dt, int(max_places), no_start_wait, fixed, listed)
    return tau, traj, recs, undecided, theirs, spots
