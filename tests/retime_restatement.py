"""A retime call (include/pp_hip.h, "decided waits written into the timetables") restated in numpy, for tests/test_gpu_pipeline_retime.py,
tests/test_retime_restatement_host.py and tests/test_retime_rule_host.py.  It shares nothing with the kernel: a profile is an [N, 3] array of (s, v, t)
rows as tests/speed_restatement.py (or the device) gives them, the stops and their arrival times are timetable_restatement.stops.  The holds of ONE
plan are (row, seconds) pairs in ascending row order; the prefix is a plain Python loop over np.float64, the rewrite one numpy addition per row, so
that every byte is the device's when it is fed the device's own rows."""
import numpy as np

import timetable_restatement as TT

MAX_HOLDS = 1 << 10
APPLIED, NO_PROFILE, NOT_A_STOP, NEGATIVE_DWELL = 0, -1, -2, -3

HOLD_DTYPE = np.dtype([("plan", np.int32), ("row", np.int32), ("seconds", np.float64)])
RESULT_DTYPE = np.dtype([("status", np.int32), ("n_holds", np.int32), ("first_row", np.int32), ("bad_hold", np.int32), ("held", np.float64), ("duration_before", np.float64),
                         ("duration", np.float64)])
assert HOLD_DTYPE.itemsize == 16 and RESULT_DTYPE.itemsize == 40


def dwell(rows, r, a_acc, a_dec):
    """delta_r = t_r - t_arrive(r) of row r >= 1 (t_arrive by the timetable restatement's formula, whether the row stands or not)"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    arrive = rows[r - 1, 2] + TT.step_time(rows[r, 0] - rows[r - 1, 0], rows[r - 1, 1], rows[r, 1], np.float64(a_acc), np.float64(a_dec))
    return rows[r, 2] - arrive


def hold_status(rows, r, seconds, a_acc, a_dec):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    if not (1 <= r < len(rows)) or rows[r, 1] != 0.0:
        return NOT_A_STOP
    return APPLIED if dwell(rows, r, a_acc, a_dec) + np.float64(seconds) >= 0.0 else NEGATIVE_DWELL


def prefix(seconds):
    """P_0 = seconds_0, P_h = P_{h-1} + seconds_h, sequentially"""
    out, total = [], None
    for w in seconds:
        total = np.float64(w) if total is None else total + np.float64(w)
        out.append(total)
    return np.array(out, dtype=np.float64)


def retime(rows, holds, a_acc, a_dec, first=0):
    """(record, rows after) of one plan: `rows` [N, 3] or None (no profile), `holds` its (row, seconds) pairs in ascending row order, `first` the index
    of its first hold in the call's list.  The rows given are not written."""
    rec = np.zeros((), dtype=RESULT_DTYPE)
    rec["bad_hold"] = -1
    if rows is None:
        rec["status"] = NO_PROFILE
        return rec, None
    rows = np.array(rows, dtype=np.float64).reshape(-1, 3)
    rec["n_holds"], rec["first_row"] = len(holds), -1
    rec["duration_before"] = rec["duration"] = rows[-1, 2]
    for k, (r, w) in enumerate(holds):
        status = hold_status(rows, int(r), w, a_acc, a_dec)
        if status != APPLIED:
            rec["status"], rec["bad_hold"] = status, first + k
            return rec, rows
    if not len(holds):
        return rec, rows
    at = np.array([int(r) for r, _ in holds])
    assert (np.diff(at) > 0).all()
    P = prefix([w for _, w in holds])
    k = np.arange(at[0], len(rows))
    h = np.searchsorted(at, k, side="right") - 1  # the last hold with row <= k
    rows[k, 2] = rows[k, 2] + P[h]
    rec["first_row"], rec["held"], rec["duration"] = at[0], P[-1], rows[-1, 2]
    return rec, rows


def retime_call(rows_of, holds, a_acc, a_dec):
    """a whole call: rows_of is a list of [N, 3] arrays (None: no profile), holds an array of HOLD_DTYPE sorted by (plan, row).  Returns (records, rows after)"""
    holds = np.asarray(holds, dtype=HOLD_DTYPE).reshape(-1)
    recs, after = np.zeros(len(rows_of), dtype=RESULT_DTYPE), []
    for i, rows in enumerate(rows_of):
        mine = np.flatnonzero(holds["plan"] == i)
        rec, new = retime(rows, [(holds["row"][k], holds["seconds"][k]) for k in mine], a_acc, a_dec, first=int(mine[0]) if len(mine) else 0)
        recs[i] = rec
        after.append(new)
    return recs, after
