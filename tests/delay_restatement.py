"""A delay call (include/pp_hip.h, "start delays that clear conflicts") restated in numpy on top of tests/conflict_restatement.py, for
tests/test_gpu_pipeline_deconflict.py, tests/test_delay_restatement_host.py and tests/test_delay_rule_host.py.  It shares nothing with the kernel or
with pp_delay_rule.hpp: the extended trajectory is conflict_restatement.trajectory over the lattice indices k0 - D .. k1, a delay is a slice of it,
and the rule -- index order, the smallest clear delay, the blocker with the least (m, j) -- is written here from the header.

A pair-time is UNDECIDED when its separation lies within EPS = 1e-9 of the margin.  A vehicle is undecided when any pair-time of a candidate it tried
(the rejected ones and the chosen one) is, and so is every vehicle below it that is reachable through pairs: records are compared on decided
vehicles only.  (Every pair-time of a tried candidate is counted, also those behind the blocker: more than the definition needs, never less.)"""
import numpy as np

import conflict_restatement as CR

EPS = CR.EPS


def partners_below(n, pairs):
    """per vehicle the list of its pair partners of smaller index, in the order of the pair list (a pair given twice is listed twice); pairs None: every pair"""
    below = [[] for _ in range(n)]
    for a, b in (CR.all_pairs(n) if pairs is None else pairs):
        a, b = int(a), int(b)
        below[max(a, b)].append(min(a, b))
    return below


def levels(n, pairs):
    """level(i) = 0 without a partner j < i, else 1 + max level(j)"""
    below = partners_below(n, pairs)
    level = [0] * n
    for i in range(n):
        level[i] = max((level[j] + 1 for j in below[i]), default=0)
    return level


def csr(n, pairs):
    """(offsets [n + 1], list) of partners_below"""
    below = partners_below(n, pairs)
    offsets = [0]
    for b in below:
        offsets.append(offsets[-1] + len(b))
    return offsets, [j for b in below for j in b]


def members_by_level(level):
    """(first [levels + 1], members): the vehicles grouped by level, ascending index within a level"""
    count = max(level) + 1 if level else 0
    members = [i for l in range(count) for i in range(len(level)) if level[i] == l]
    first = [0]
    for l in range(count):
        first.append(first[-1] + sum(1 for x in level if x == l))
    return first, members


def column(m, D, d):
    """the column of the extended trajectory a vehicle delayed by d steps is at, at lattice time k0 + m"""
    return m + D - d


def key(m, n, j):
    return m * n + j


def separations(ca, cb, radius):
    """the separation per time of two vehicles whose disc centres are ca, cb [K, m, 2]: the minimum over disc pairs"""
    sep = np.full(ca.shape[1], np.inf)
    for a in range(len(radius)):
        for b in range(len(radius)):
            dx, dy = ca[a, :, 0] - cb[b, :, 0], ca[a, :, 1] - cb[b, :, 1]
            sep = np.minimum(sep, np.sqrt(dx * dx + dy * dy) - (radius[a] + radius[b]))
    return sep


def decide(traj, s_of, tau, T, D, n, pairs, discs, margin, t_start, dt):
    """the records of a delay call from the extended trajectories: traj[i] is conflict_restatement.trajectory's dict over T + D columns (status, present,
    poses), s_of[i] the arc lengths per column; tau the T lattice times of the call"""
    below = partners_below(n, pairs)
    radius = np.array([np.float64(np.float32(r)) for _, _, r in discs])
    margin = np.float64(margin)
    centre = [CR.centres(np.nan_to_num(t["poses"]), discs) if t["status"] >= 0 else None for t in traj]
    m_all = np.arange(T)
    delay, recs = [-1] * n, []
    for i in range(n):
        rec = dict(status=-1, delay_steps=-1, n_tried=0, blocker=-1, t_start=0.0, t_block=0.0, s_block=(0.0, 0.0), undecided=False)
        recs.append(rec)
        if traj[i]["status"] < 0:
            continue
        rec["undecided"] = any(recs[j]["undecided"] for j in below[i])
        blocked = None
        for d in range(D + 1):
            ci = column(m_all, D, d)
            best = None
            for j in sorted(set(below[i])):
                if delay[j] < 0:
                    continue
                cj = column(m_all, D, delay[j])
                both = np.flatnonzero(traj[i]["present"][ci] & traj[j]["present"][cj])
                if not len(both):
                    continue
                sep = separations(centre[i][:, ci[both]], centre[j][:, cj[both]], radius)
                if (np.abs(sep - margin) <= EPS).any():
                    rec["undecided"] = True
                hit = np.flatnonzero(sep < margin)
                if len(hit):
                    k = key(int(both[hit[0]]), n, j)
                    best = k if best is None or k < best else best
            rec["n_tried"] += 1
            if best is None:
                rec.update(status=0, delay_steps=d, t_start=float(np.float64(t_start[i]) + np.float64(d) * np.float64(dt)))
                delay[i] = d
                break
            blocked = (best // n, best % n, d)
        else:
            rec.update(status=1, t_start=float(t_start[i]))
        if blocked is not None:
            m, j, d = blocked
            rec.update(blocker=j, t_block=float(tau[m]), s_block=(float(s_of[i][column(m, D, d)]), float(s_of[j][column(m, D, delay[j])])))
    return recs


def deconflict(plans, rows, t_start, pairs, discs, a_acc, a_dec, t_from, t_to, dt, margin=0.0, hold_before=False, hold_after=False, max_delay_steps=0, poses=None):
    """(tau, extended trajectories, records) of a whole call; pairs None: every pair.  poses (a list of [T + D, 3] arrays, NaN where absent): the
    extended trajectories' poses and presence are taken from there, not restated (the bit-exact mode of the GPU test: the device's own poses)"""
    k0, T = CR.lattice(t_from, t_to, dt)
    D = int(max_delay_steps)
    assert 1 <= T and D >= 0 and T + D <= CR.MAX_TIMES
    tau, extended = CR.times(k0, T, dt), CR.times(k0 - D, T + D, dt)
    traj = [CR.trajectory(p, r, t0, extended, a_acc, a_dec, hold_before, hold_after) for p, r, t0 in zip(plans, rows, t_start)]
    if poses is not None:
        for t, xyt in zip(traj, poses):
            if t["status"] >= 0:
                t["poses"], t["present"] = np.asarray(xyt, dtype=np.float64), ~np.isnan(np.asarray(xyt)[:, 0])
    s_of = [t.get("s") for t in traj]
    return tau, traj, decide(traj, s_of, tau, T, D, len(plans), pairs, discs, margin, t_start, dt)
