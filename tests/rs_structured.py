"""Structured Reeds-Shepp inputs (no test functions): the poses a planner is really fed -- round coordinates, headings on multiples of pi/4,
goals exactly ahead or exactly 2 or 4 turning radii away -- where the solver's arithmetic sits on a knife edge (acos(1), sqrt(0), asin(x / 0),
mirrored words of bit-identical cost, motions of length exactly 0), and the tools the tests on them share:

  structured_pairs(rmin)   the pose pairs, in a fixed order
  flagged(a, b, rmin, c)   the oracle-only fragility probe: does the winning word change when one input coordinate moves by one ulp?
  integrate(...)           what a path record MEANS, stated independently of the oracle: arcs rotate about their centre, straights translate
  junction_ratios(P)       the ratios at which Interpolate / Truncate / GetDirection change motion, with their float neighbours
  query_candidates(...), stable_queries(...)   structured near-goal search queries, the oracle-only selection of the reproducible ones
"""
import math

import numpy as np

import oracle_lib as O

COSTS = [(1.0, 1.0, 0.0), (2.0, 1.0, 0.5), (1.0, 1.5, 0.0)]  # (reverse, forward, switch)

OFFSETS = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0, 6.0, -6.0, 8.0, -8.0])  # in turning radii, on each axis
HEADINGS = np.arange(-4, 5) * (math.pi / 4)  # k * pi / 4, -pi and +pi both
ORIGINS = ((0.0, 0.0), (3.0, -7.0))
N_GRID = len(ORIGINS) * len(HEADINGS) * len(OFFSETS) * len(OFFSETS) * len(HEADINGS)  # 36 450
N_UNWRAPPED = 64
N_NEAR_OFFSET = 64


def structured_pairs(rmin):
    """-> (a, b): [n, 3] starts and goals.  The grid (origin x start heading x goal offset x, y x goal heading, 36 450 pairs), then 64 grid
    pairs whose start heading is unwrapped by +-2 pi, then 64 whose goal lies 1e-9 * rmin or 1e-12 * rmin from its offset."""
    o, ts, ox, oy, tg = np.meshgrid(np.arange(len(ORIGINS)), HEADINGS, OFFSETS * rmin, OFFSETS * rmin, HEADINGS, indexing="ij")
    org = np.array(ORIGINS)[o.reshape(-1)]
    a = np.column_stack([org[:, 0], org[:, 1], ts.reshape(-1)])
    b = np.column_stack([org[:, 0] + ox.reshape(-1), org[:, 1] + oy.reshape(-1), tg.reshape(-1)])
    assert len(a) == N_GRID
    pick = (np.arange(N_UNWRAPPED) * 569 + 11) % N_GRID  # spread over origins, headings and offsets
    ua, ub = a[pick].copy(), b[pick].copy()
    ua[:, 2] += np.where(np.arange(N_UNWRAPPED) % 2 == 0, 2 * math.pi, -2 * math.pi)
    pick = (np.arange(N_NEAR_OFFSET) * 571 + 29) % N_GRID
    na, nb = a[pick].copy(), b[pick].copy()
    k = np.arange(N_NEAR_OFFSET)
    eps = np.where(k % 2 == 0, 1e-9, 1e-12) * rmin * np.where((k // 2) % 2 == 0, 1.0, -1.0)
    axis = (k // 4) % 2
    nb[k, axis] += eps
    return np.concatenate([a, ua, na]), np.concatenate([b, ub, nb])


def nudges(a, b):
    """the 12 copies of (a, b) with one of the six coordinates moved to its float neighbour, up and down"""
    for which, col in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)):
        for toward in (np.inf, -np.inf):
            pair = [a.copy(), b.copy()]
            pair[which][:, col] = np.nextafter(pair[which][:, col], toward)
            yield pair[0], pair[1]


def relative_pose(a, b):
    """the goal in the start's frame, as the solver forms it before it normalises by the turning radius (heading not wrapped here: the
    solver wraps it).  numpy's sin / cos need not be the oracle's to the last bit; the probe nudges these values anyway."""
    dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    s, c = np.sin(-a[:, 2]), np.cos(-a[:, 2])
    return np.column_stack([c * dx + (-s) * dy, s * dx + c * dy, b[:, 2] - a[:, 2]])


def flagged(a, b, rmin, costs):
    """The oracle-only fragility probe.  -> (mask [n] bool, seen [n, 48] bool): seen[i, w] when word w wins pair i in the plain run, in
    one of the 12 one-ulp nudges of a coordinate of start or goal, or -- solved from the origin, where the solver's own frame change is
    exact -- at the relative pose and its 6 one-ulp nudges; mask[i] when more than one word is seen.  Wherever a last bit of an INPUT
    decides the word, a last bit of libm may too, and another implementation is entitled to any word of the set.  The relative pose is
    nudged because the world coordinates cannot reach every neighbour of it: sin and cos of a heading on a multiple of pi / 2 swallow a
    one-ulp change of the heading, and a product with 6e-17 swallows one of an offset."""
    rev, fwd, sw = costs
    word = O.rs_optimal_batch(a, b, rmin, rev, fwd, sw)[0]
    seen = np.zeros((len(a), 48), bool)
    rows = np.arange(len(a))
    seen[rows[word >= 0], word[word >= 0]] = True
    mask = np.zeros(len(a), bool)
    rel = relative_pose(a, b)
    runs = list(nudges(a, b)) + [(np.zeros_like(rel), rel)] + [(np.zeros_like(rel), nb) for na, nb in list(nudges(rel, rel))[6:]]
    for na, nb in runs:
        w = O.rs_optimal_batch(na, nb, rmin, rev, fwd, sw)[0]
        mask |= w != word
        seen[rows[w >= 0], w[w >= 0]] = True
    return mask, seen


def mirror_ties(a, b, rmin, costs, word, cost):
    """Pairs with two words of bit-identical float cost, shown on the oracle alone: the whole problem mirrored in the start's x axis
    (y and both headings negated -- exact in floating point, so the 48 candidate costs are the same numbers under the permutation
    word -> word ^ 2) must return the same float cost; where it does NOT return the mirror image of the pair's word, the pair's word and
    that other word tie exactly, and word order alone decided."""
    am, bm = a.copy(), b.copy()
    am[:, 2] = -a[:, 2]
    bm[:, 1] = 2 * a[:, 1] - b[:, 1]
    bm[:, 2] = -b[:, 2]
    exact = (bm[:, 1] - am[:, 1]) == -(b[:, 1] - a[:, 1])
    w2, _, cost2, _ = O.rs_optimal_batch(am, bm, rmin, *costs)
    assert np.array_equal(cost2[exact], cost[exact])
    return exact & ((w2 ^ 2) != word)


# ------------------------------------------------------------------------------------------------------ integrate --
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 1.1e-19)
LEFT, STRAIGHT, RIGHT = 0, 1, 2
FORWARD, BACKWARD, NO_MOTION = 0, 1, 2


def _integrate_longdouble(start, steer, direction, motion_length, rmin):
    ld = np.longdouble
    x, y, t = (np.asarray(start)[:, k].astype(ld) for k in range(3))
    r = ld(rmin)
    live = np.ones(len(x), bool)
    for i in range(motion_length.shape[1]):
        live = live & (direction[:, i] != NO_MOTION) & np.isfinite(motion_length[:, i])  # the motions up to the first unused slot
        l = np.where(live, motion_length[:, i], 0.0).astype(ld) * np.where(direction[:, i] == BACKWARD, ld(-1), ld(1))
        s = steer[:, i]
        turn = live & (s != STRAIGHT)
        side = np.where(s == RIGHT, ld(-1), ld(1))  # the centre lies to the left (+) or right (-) of the heading
        cx, cy = x - side * r * np.sin(t), y + side * r * np.cos(t)
        t2 = t + side * l
        ax, ay = cx + side * r * np.sin(t2), cy - side * r * np.cos(t2)
        sx, sy = x + l * r * np.cos(t), y + l * r * np.sin(t)
        x, y, t = np.where(turn, ax, np.where(live, sx, x)), np.where(turn, ay, np.where(live, sy, y)), np.where(turn, t2, t)
    return np.column_stack([x, y, t])


def _integrate_mpmath(start, steer, direction, motion_length, rmin, rows):
    import mpmath
    out = np.full((len(start), 3), np.nan, np.longdouble)
    with mpmath.workdps(40):
        r = mpmath.mpf(float(rmin))
        for q in rows:
            x, y, t = (mpmath.mpf(float(v)) for v in start[q])
            for i in range(motion_length.shape[1]):
                if direction[q, i] == NO_MOTION or not np.isfinite(motion_length[q, i]):
                    break
                l = mpmath.mpf(float(motion_length[q, i])) * (-1 if direction[q, i] == BACKWARD else 1)
                if steer[q, i] == STRAIGHT:
                    x, y = x + l * r * mpmath.cos(t), y + l * r * mpmath.sin(t)
                else:
                    side = -1 if steer[q, i] == RIGHT else 1
                    cx, cy = x - side * r * mpmath.sin(t), y + side * r * mpmath.cos(t)
                    t = t + side * l
                    x, y = cx + side * r * mpmath.sin(t), cy - side * r * mpmath.cos(t)
            out[q] = [np.longdouble(float(v)) + np.longdouble(float(v - float(v))) for v in (x, y, t)]  # (two doubles: nothing rounded away)
    return out


def integrate(start, steer, direction, motion_length, rmin, must=None):
    """The end pose of a path record by a plain closed-form walk of its motions: a left / right arc of angle motion_length rotates the pose
    about the centre rmin to its left / right, a straight motion translates it by motion_length * rmin, backward negates.  Headings are not
    wrapped.  numpy.longdouble where that is the 64-bit-mantissa format; otherwise mpmath at 40 digits on the rows `must` (bool mask: the
    flagged pairs and those with a zero or tiny motion) and on every 16th of the rest -- the other rows come back NaN and pose_error()
    leaves them out.  -> [n, 3] longdouble."""
    start = np.asarray(start, np.float64).reshape(-1, 3)
    steer, direction, motion_length = np.asarray(steer), np.asarray(direction), np.asarray(motion_length, np.float64)
    if LONGDOUBLE_OK:
        return _integrate_longdouble(start, steer, direction, motion_length, rmin)
    rows = np.zeros(len(start), bool)
    rows[::16] = True
    if must is not None:
        rows |= must
    return _integrate_mpmath(start, steer, direction, motion_length, rmin, np.flatnonzero(rows))


def integrate_records(P, must=None):
    """integrate() of path records (oracle_lib.RS_PATH_DTYPE) that share one turning radius"""
    rmin = float(P["min_turning_radius"][0]) if len(P) else 1.0
    assert (P["min_turning_radius"] == rmin).all()
    return integrate(P["start"], P["steer"], P["direction"], P["motion_length"], rmin, must)


def pose_error(got, want):
    """largest of |dx|, |dy| and |dtheta| modulo 2 pi per row (float64); rows that integrate() left out (NaN) count 0"""
    ld = np.longdouble
    d = np.asarray(got, ld) - np.asarray(want, ld)
    two_pi = ld(8) * np.arctan(ld(1))
    d[:, 2] = d[:, 2] - two_pi * np.rint(d[:, 2] / two_pi)
    e = np.abs(d).max(axis=1)
    return np.where(np.isnan(e), 0.0, e).astype(np.float64)


def zero_or_tiny(P):
    """-> (has a motion of length exactly 0, has a motion with 0 < |l| < 1e-9) per record, among the used slots"""
    used = (P["direction"] != NO_MOTION) & np.isfinite(P["motion_length"])
    l = np.abs(np.where(used, P["motion_length"], 1.0))
    return (l == 0.0).any(axis=1), ((l > 0.0) & (l < 1e-9)).any(axis=1)


def record_length(P, used):
    """PathSegment::AddMotion's running sum of |motion_length| in slot order, times the turning radius"""
    total = np.zeros(len(P))
    for i in range(5):
        total = total + np.where(used[:, i], np.abs(P["motion_length"][:, i]), 0.0)
    return total * P["min_turning_radius"]


# ------------------------------------------------------------------------------------------- headings at +-pi --
PI_BAND = 1e-9


def fold_pi(theta):
    """Headings within PI_BAND below +pi moved to the same angle next to -pi.  WrapTheta leaves +pi and -pi both in place, so a heading
    that arrives at pi by a sum of turn angles comes out as +pi or as -pi by the last bit of that sum -- the same angle, 2 pi apart as
    numbers.  Half the structured goals face that way.  A tolerance on such a heading is meant across the cut: both sides of a comparison
    go through this, and the tolerance itself stays what it was."""
    theta = np.array(theta, dtype=np.float64, copy=True)
    return np.where(theta > math.pi - PI_BAND, theta - 2 * math.pi, theta)


def folded(records):
    """path records with the heading of final_pose through fold_pi (a copy)"""
    out = np.array(records, copy=True)
    out["final_pose"][:, 2] = fold_pi(out["final_pose"][:, 2])
    return out


def folded_poses(poses):
    out = np.array(poses, dtype=np.float64, copy=True)
    out[:, 2] = fold_pi(out[:, 2])
    return out


# ------------------------------------------------------------------------------------------------ junction ratios --
def junction_ratios(P):
    """[n, 17]: per record the cumulative motion_length[i] * rmin / length behind each of the five slots -- len += motion_length[i] * rmin;
    ratio = len / length, in float64 as PathReedsShepp does it -- each with its float neighbour above and below, then 0 and 1.  These are
    the ratios at which `len >= ratio * totalLength` and `ratio * length <= len` decide.  Unused slots and zero-length paths give 0.5."""
    P = np.asarray(P).reshape(-1)
    n = len(P)
    out = np.full((n, 17), 0.5)
    length = P["length"]
    rmin = P["min_turning_radius"]
    acc = np.zeros(n)
    live = length != 0.0
    for i in range(5):
        live = live & (P["direction"][:, i] != NO_MOTION) & np.isfinite(P["motion_length"][:, i])
        acc = acc + np.where(live, P["motion_length"][:, i], 0.0) * rmin
        with np.errstate(invalid="ignore", divide="ignore"):
            r = acc / length
        ok = live & np.isfinite(r)
        out[ok, 3 * i] = r[ok]
        out[ok, 3 * i + 1] = np.nextafter(r[ok], np.inf)
        out[ok, 3 * i + 2] = np.nextafter(r[ok], -np.inf)
    out[:, 15] = 0.0
    out[:, 16] = 1.0
    return out


# ------------------------------------------------------------------------------------------------- search queries --
QUERY_OFFSETS = ((4, 0), (0, 4), (4, 4), (-4, 0), (6, 2), (2, -6), (-4, 4), (8, 0), (0, -8), (4, -2), (-6, 0), (2, 2))
N_QUERY_CANDIDATES = 38
QUERY_SEED0 = 700


def query_candidates(valid, count, span=6):
    """structured near-goal queries in a fixed order (valid(poses) -> bool per pose: the map's verdict): starts at
    (i + 0.37, j + 0.21, k pi / 2 - pi) for integer i, j within `span` of the centre, goal = start o offset (QUERY_OFFSETS in turn, rotated by the start heading), goal headings stepping by pi / 2;
    both poses valid.  The 0.37 / 0.21 shift keeps the starts off the lattice lines."""
    starts, goals = [], []
    c = 0
    for i in range(-span, span + 1):
        for j in range(-span, span + 1):
            k = c % 4
            ox, oy = QUERY_OFFSETS[c % len(QUERY_OFFSETS)]
            t = k * (math.pi / 2) - math.pi
            s = np.array([i + 0.37, j + 0.21, t])
            g = np.array([s[0] + ox * math.cos(t) - oy * math.sin(t), s[1] + ox * math.sin(t) + oy * math.cos(t), t + ((c // 4) % 4) * (math.pi / 2)])
            c += 1
            if valid(np.array([s, g])).all():
                starts.append(s)
                goals.append(g)
                if len(starts) == count:
                    return np.array(starts), np.array(goals)
    return np.array(starts), np.array(goals)


def search_signature(r):
    return (r["status"], len(r["expanded"]), r["n_rs_attempts"], tuple(r["path_kind"]), tuple(r["path_rsword"]))


def stable_queries(h, starts, goals, seeds):
    """the oracle-only selection: query q is kept when (status, n_expanded, n_rs_attempts, path_kind, path_rsword) of the oracle's search
    is the same under the 12 one-ulp nudges of its start and goal.  -> (kept indices, the oracle's results of the kept queries)"""
    kept, results = [], []
    for q in range(len(starts)):
        r = h.search(starts[q], goals[q], int(seeds[q]))
        sig = search_signature(r)
        if all(search_signature(h.search(na[0], nb[0], int(seeds[q]))) == sig for na, nb in nudges(starts[q:q + 1], goals[q:q + 1])):
            kept.append(q)
            results.append(r)
    if len(kept) % 4 == 0:  # a count that is no multiple of four: the last wave of the rows kernels has idle rows
        kept, results = kept[:-1], results[:-1]
    return np.array(kept, dtype=np.int64), results


def assert_queries_exercise_the_attempt(results, goals, min_ties=2):
    """what the kept queries must hold for the search tests to mean something; among them plans whose last edge was picked from two
    words of bit-identical cost (mirror_ties on the edge's parent pose and the goal, default parameters: rmin 2, unit costs)"""
    assert len(results) >= 16 and len(results) % 4 != 0, len(results)
    assert sum(r["status"] == 0 and len(r["path_kind"]) == 2 and r["path_kind"][-1] == 2 for r in results) >= 4  # one-edge plans
    assert sum(r["n_rs_attempts"] > 1 for r in results) >= 6  # attempts the march rejected
    edge_from = np.array([r["path_poses"][-2] for r in results])
    word, _, cost, _ = O.rs_optimal_batch(edge_from, goals, 2.0)
    assert np.array_equal(word, [r["path_rsword"][-1] for r in results])
    ties = mirror_ties(edge_from, goals, 2.0, COSTS[0], word, cost)
    assert ties.sum() >= min_ties
    return ties
