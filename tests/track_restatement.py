"""A delay call with tracked movers (include/pp_hip.h, "start delays that clear conflicts and tracked movers") restated in numpy on top of
tests/conflict_restatement.py, for tests/test_gpu_pipeline_deconflict_tracks.py, tests/test_track_restatement_host.py and
tests/test_track_rule_host.py.  It shares nothing with the kernels or with pp_track_rule.hpp: the extended trajectory is
conflict_restatement.trajectory over the lattice indices k0 - D .. k1, a delay is a slice of it, and the track samples (one correctly rounded
double operation per step, in the header's order), the combined rule -- index order, the smallest delay clear of the scheduled partners above and
of every track, the blocker with the least key m * (n + M) + partner -- and the (vehicle, track) records are written here from the header.

A pair-time is UNDECIDED when its separation lies within EPS = 1e-9 of the margin.  A vehicle is undecided when any pair-time of a candidate it tried
(against a vehicle or a track) is, and so is every vehicle below it that is reachable through pairs, as in tests/delay_restatement.py.  A (vehicle,
track) record is undecided when its vehicle is, or one of the record's own times is."""
import math

import numpy as np

import conflict_restatement as CR

EPS = CR.EPS


def waypoint_of(t, tau):
    """the largest j with t_j <= tau (t strictly increasing, t_0 <= tau)"""
    return np.clip(np.searchsorted(np.asarray(t, dtype=np.float64), tau, side="right") - 1, 0, len(t) - 1)


def track_position(waypoints, tau):
    """(present [m] bool, xy [m, 2], NaN where absent) of the track with rows (t, x, y) at the times tau"""
    w, tau = np.asarray(waypoints, dtype=np.float64).reshape(-1, 3), np.asarray(tau, dtype=np.float64)
    t, x, y = w[:, 0], w[:, 1], w[:, 2]
    W = len(w)
    present = ~((tau < t[0]) | (tau > t[-1]))
    j = waypoint_of(t, tau)
    j1 = np.minimum(j + 1, W - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = (tau - t[j]) / (t[j1] - t[j])
        px = np.where(j == W - 1, x[j], x[j] + lam * (x[j1] - x[j]))
        py = np.where(j == W - 1, y[j], y[j] + lam * (y[j1] - y[j]))
    xy = np.stack([px, py], axis=1)
    xy[~present] = np.nan
    return present, xy


def partner_of_track(n, k):
    return n + k


def key(m, n, M, partner):
    return m * (n + M) + partner


def partners_below(n, pairs):
    """per vehicle its pair partners of smaller index; pairs None: every pair"""
    below = [[] for _ in range(n)]
    for a, b in (CR.all_pairs(n) if pairs is None else pairs):
        a, b = int(a), int(b)
        below[max(a, b)].append(min(a, b))
    return below


def vehicle_separations(ca, cb, radius):
    """two vehicles whose disc centres are ca, cb [K, m, 2]: per time the minimum over disc pairs"""
    sep = np.full(ca.shape[1], np.inf)
    for a in range(len(radius)):
        for b in range(len(radius)):
            dx, dy = ca[a, :, 0] - cb[b, :, 0], ca[a, :, 1] - cb[b, :, 1]
            sep = np.minimum(sep, np.sqrt(dx * dx + dy * dy) - (radius[a] + radius[b]))
    return sep


def track_separations(ca, xy, radius, R):
    """a vehicle whose disc centres are ca [K, m, 2] and a track at xy [m, 2] with radius R: per time the minimum over the vehicle's discs"""
    sep = np.full(ca.shape[1], np.inf)
    for a in range(len(radius)):
        dx, dy = ca[a, :, 0] - xy[:, 0], ca[a, :, 1] - xy[:, 1]
        sep = np.minimum(sep, np.sqrt(dx * dx + dy * dy) - (radius[a] + np.float64(R)))
    return sep


def track_record(vehicle, status, candidate, s, centre, tau, T, D, sampled, R, radius, margin):
    """the record of one vehicle against one track at the vehicle's reported candidate"""
    zero = dict(n_times=0, n_conflict=0, t_first=0.0, s_first=0.0, min_separation=0.0, t_min=0.0, s_min=0.0, undecided=False)
    if status < 0:
        return dict(zero, status=-1)
    present_k, xy = sampled
    c = np.arange(T) + D - candidate
    both = np.flatnonzero(vehicle["present"][c] & present_k)
    if len(both) == 0:
        return dict(zero, status=2, min_separation=math.inf)
    sep = track_separations(centre[:, c[both]], xy[both], radius, R)
    conflict = sep < margin
    k = int(np.argmin(sep))  # (the first of equals: the smallest tau)
    rec = dict(zero, status=1 if conflict.any() else 0, n_times=len(both), n_conflict=int(conflict.sum()), min_separation=float(sep[k]), t_min=float(tau[both[k]]),
               s_min=float(s[c[both[k]]]), undecided=bool((np.abs(sep - margin) <= EPS).any()))
    if conflict.any():
        f = both[int(np.argmax(conflict))]
        rec.update(t_first=float(tau[f]), s_first=float(s[c[f]]))
    return rec


def decide(traj, s_of, tau, T, D, n, pairs, discs, margin, t_start, dt, tracks):
    """(delay records, [n][M] track records) from the extended trajectories (conflict_restatement.trajectory's dicts over T + D columns, s_of[i] the arc
    lengths per column) and the tracks [(radius, waypoints)]"""
    below = partners_below(n, pairs)
    M = len(tracks)
    radius = np.array([np.float64(np.float32(r)) for _, _, r in discs])
    margin = np.float64(margin)
    centre = [CR.centres(np.nan_to_num(t["poses"]), discs) if t["status"] >= 0 else None for t in traj]
    sampled = [track_position(w, tau) for _, w in tracks]
    m_all = np.arange(T)
    delay, recs, track_recs = [-1] * n, [], []
    for i in range(n):
        rec = dict(status=-1, delay_steps=-1, n_tried=0, blocker=-1, t_start=0.0, t_block=0.0, s_block=(0.0, 0.0), undecided=False)
        recs.append(rec)
        if traj[i]["status"] < 0:
            track_recs.append([track_record(None, -1, 0, None, None, tau, T, D, None, 0.0, radius, margin) for _ in range(M)])
            continue
        rec["undecided"] = any(recs[j]["undecided"] for j in below[i])
        blocked = None
        for d in range(D + 1):
            ci = m_all + D - d
            best = None
            for j in sorted(set(below[i])):
                if delay[j] < 0:
                    continue
                cj = m_all + D - delay[j]
                both = np.flatnonzero(traj[i]["present"][ci] & traj[j]["present"][cj])
                if not len(both):
                    continue
                sep = vehicle_separations(centre[i][:, ci[both]], centre[j][:, cj[both]], radius)
                if (np.abs(sep - margin) <= EPS).any():
                    rec["undecided"] = True
                hit = np.flatnonzero(sep < margin)
                if len(hit):
                    k = key(int(both[hit[0]]), n, M, j)
                    best = k if best is None or k < best else best
            for t, (R, _) in enumerate(tracks):
                present_t, xy = sampled[t]
                both = np.flatnonzero(traj[i]["present"][ci] & present_t)
                if not len(both):
                    continue
                sep = track_separations(centre[i][:, ci[both]], xy[both], radius, R)
                if (np.abs(sep - margin) <= EPS).any():
                    rec["undecided"] = True
                hit = np.flatnonzero(sep < margin)
                if len(hit):
                    k = key(int(both[hit[0]]), n, M, partner_of_track(n, t))
                    best = k if best is None or k < best else best
            rec["n_tried"] += 1
            if best is None:
                rec.update(status=0, delay_steps=d, t_start=float(np.float64(t_start[i]) + np.float64(d) * np.float64(dt)))
                delay[i] = d
                break
            blocked = (best // (n + M), best % (n + M), d)
        else:
            rec.update(status=1, t_start=float(t_start[i]))
        if blocked is not None:
            m, j, d = blocked
            rec.update(blocker=j, t_block=float(tau[m]), s_block=(float(s_of[i][m + D - d]), float(s_of[j][m + D - delay[j]]) if j < n else 0.0))
        candidate = rec["delay_steps"] if rec["status"] == 0 else D
        row = [track_record(traj[i], rec["status"], candidate, s_of[i], centre[i], tau, T, D, sampled[t], R, radius, margin) for t, (R, _) in enumerate(tracks)]
        for r in row:
            r["undecided"] = r["undecided"] or rec["undecided"]
        track_recs.append(row)
    return recs, track_recs


def deconflict_tracks(plans, rows, t_start, pairs, discs, a_acc, a_dec, tracks, t_from, t_to, dt, margin=0.0, hold_before=False, hold_after=False, max_delay_steps=0,
                      poses=None):
    """(tau, extended trajectories, delay records, track records) of a whole call; pairs None: every pair; tracks: [(radius, waypoints [W, 3])].  poses (a
    list of [T + D, 3] arrays, NaN where absent): the extended trajectories' poses and presence are taken from there, not restated (the bit-exact mode of
    the GPU test: the device's own poses)"""
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
    tracks = [] if tracks is None else [(float(R), np.asarray(w, dtype=np.float64).reshape(-1, 3)) for R, w in tracks]
    recs, track_recs = decide(traj, s_of, tau, T, D, len(plans), pairs, discs, margin, t_start, dt, tracks)
    return tau, traj, recs, track_recs
