"""The two stages of a locate call (include/pp_hip.h, "locating vehicles on held plans") restated in numpy, for tests/test_gpu_pipeline_locate.py
and tests/test_locate_restatement_host.py.  It shares nothing with the kernel: a plan is a list of edge objects that give their own poses
(constant-steer arcs from the closed form in numpy; Reeds-Shepp edges through whatever interpolates their records -- pp_rs_path_interpolate on the
GPU box, the oracle on the CPU); the schedule, the cost, the order, the lattice and the arc length -> (edge, ratio) mapping are written here from
the definition.

A case is DECIDED when the best candidate beats, by more than EPS = 1e-9 m^2, every other stage-2 candidate and every stage-1 sample farther than
2 * spacing from it.  (Device and glibc poses differ around 1e-12 m; with a lever of 40 m that is 1e-10 m^2.)  "Other" means another point of the plan:
a candidate with the best's own arc length is the best's own point (the lattice point 0 under the first sample: the same edge, ratio and pose)."""
import math

import numpy as np

TWO_PI = 6.283185307179586
EPS = 1e-9
MAX_STEPS = 1 << 19


def steps(L, spacing):
    if not L > 0.0:
        return 0
    q = L / spacing
    return MAX_STEPS if not q < MAX_STEPS else int(math.ceil(q))


class ArcEdge:
    """ConstantSteer from `start` over L metres with curvature kappa (kinematic_bicycle_model.cpp:5-32)"""

    def __init__(self, start, L, kappa, backward):
        self.start, self.L, self.kappa, self.backward = np.array(start, dtype=np.float64), float(L), float(kappa), bool(backward)

    def at(self, ratio):
        x0, y0, t0 = self.start
        d = self.L * np.asarray(ratio, dtype=np.float64)
        if self.backward:
            d = -d
        if abs(self.kappa) > 1e-9:
            t = t0 + d * self.kappa
            poses = np.column_stack([x0 + 1 / self.kappa * (np.sin(t) - math.sin(t0)), y0 + 1 / self.kappa * (-np.cos(t) + math.cos(t0)), t])
        else:
            poses = np.column_stack([x0 + d * math.cos(t0), y0 + d * math.sin(t0), np.full(len(d), t0)])
        return poses, np.full(len(d), -1 if self.backward else 1)


class RsEdge:
    """a Reeds-Shepp record (RS_PATH_DTYPE, one element) evaluated by interpolate(records, ratios) -> (poses, directions 0 forward / 1 backward)"""

    def __init__(self, record, L, interpolate):
        self.record, self.L, self.interpolate = record, float(L), interpolate

    def at(self, ratio):
        ratio = np.ascontiguousarray(ratio, dtype=np.float64)
        poses, direction = self.interpolate(np.repeat(self.record, len(ratio)), ratio)
        return poses, np.where(direction == 1, -1, 1)


class Plan:
    """first: the pose of node 0; edges: root first (none: a one-pose plan)"""

    def __init__(self, first, edges):
        self.first, self.edges = np.array(first, dtype=np.float64), list(edges)
        self.L = np.array([e.L for e in self.edges], dtype=np.float64)
        S, total = [], 0.0
        for e in self.edges:  # the sequential root-first sum
            S.append(total)
            total = total + e.L
        self.S, self.length = np.array(S, dtype=np.float64), total
        self._samples = {}

    def samples(self, spacing):
        """stage 1's schedule: (edge [m], ratio [m], s [m], poses [m, 3], direction [m]), edge after edge"""
        if spacing not in self._samples:
            edge, ratio, arc, poses, direction = [], [], [], [], []
            for e, E in enumerate(self.edges, start=1):
                n = steps(E.L, spacing)
                r = np.arange(n + 1, dtype=np.float64) / np.float64(n) if n else np.zeros(1)
                p, d = E.at(r)
                edge.append(np.full(len(r), e))
                ratio.append(r)
                arc.append(self.S[e - 1] + r * E.L)
                poses.append(p)
                direction.append(d)
            self._samples[spacing] = tuple(np.concatenate(x) for x in (edge, ratio, arc, poses, direction))
        return self._samples[spacing]

    def at(self, edge, ratio):
        """poses and directions at (edge[k], ratio[k])"""
        edge, ratio = np.asarray(edge), np.asarray(ratio, dtype=np.float64)
        poses, direction = np.empty((len(edge), 3)), np.empty(len(edge), dtype=np.int64)
        for e in np.unique(edge):
            k = edge == e
            poses[k], direction[k] = self.edges[e - 1].at(ratio[k])
        return poses, direction


def errors(v, poses):
    ex, ey, a = v[0] - poses[:, 0], v[1] - poses[:, 1], v[2] - poses[:, 2]
    return ex, ey, a - TWO_PI * np.rint(a / TWO_PI)


def cost(v, poses, w):
    ex, ey, d = errors(v, poses)
    return (ex * ex + ey * ey) + (w * d) * (w * d)


def first_best(c, s):
    """index of the least (c, s), the first of equals"""
    k = np.flatnonzero(c == c.min())
    return int(k[np.argmin(s[k])])  # (argmin: the first of equals)


def locate(plan, vehicle, spacing, w=0.0, lo=-np.inf, hi=np.inf):
    """the record a locate call owes for `plan` (None: no plan) and the vehicle pose, as a dict; for status 0 also `decided`, `c` (the least cost)
    and `cost_at(edge, ratio)`"""
    zero = dict(edge=0, direction=0, s=0.0, ratio=0.0, distance=0.0, along=0.0, lateral=0.0, heading_error=0.0, pose=(0.0, 0.0, 0.0))
    if plan is None:
        return dict(zero, status=-1, n_samples=0, length=0.0)
    v = np.array(vehicle, dtype=np.float64)

    def record(edge, direction, s, ratio, pose, n_samples, decided, cost_at):
        ex, ey, d = (float(x[0]) for x in errors(v, pose[None]))
        cs, sn = math.cos(pose[2]), math.sin(pose[2])
        return dict(status=0, n_samples=n_samples, length=plan.length, edge=int(edge), direction=int(direction), s=float(s), ratio=float(ratio), pose=tuple(float(x) for x in pose),
                    distance=math.sqrt(ex * ex + ey * ey), along=cs * ex + sn * ey, lateral=cs * ey - sn * ex, heading_error=d, decided=decided,
                    c=float(cost(v, pose[None], w)[0]), cost_at=cost_at)

    if not plan.edges:  # one sample: the pose, at s = 0; no second stage
        if not (0.0 >= lo and 0.0 <= hi):
            return dict(zero, status=1, n_samples=0, length=0.0)
        return record(0, 1, 0.0, 0.0, plan.first, 1, True, lambda edge, ratio: float(cost(v, plan.first[None], w)[0]))
    # ---- stage 1
    edge, ratio, arc, poses, direction = plan.samples(spacing)
    keep = (arc >= lo) & (arc <= hi)
    if not keep.any():
        return dict(zero, status=1, n_samples=0, length=plan.length)
    c1 = cost(v, poses, w)
    # (a junction pose is sampled twice at one arc length: the start of the later edge is the candidate, the end of the earlier one only counts)
    inside = np.flatnonzero(keep & ~((ratio == 1.0) & (edge < len(plan.edges))))
    k1 = int(inside[first_best(c1[inside], arc[inside])])
    s1 = arc[k1]
    # ---- stage 2: the global lattice around s1
    delta = spacing / 32.0
    i = np.int64(math.floor(s1 / delta)) + np.arange(-32, 34, dtype=np.int64)
    u = i.astype(np.float64) * delta
    u = u[(u >= 0.0) & (u <= plan.length) & (u >= lo) & (u <= hi)]
    e2 = np.searchsorted(plan.S, u, side="right")  # the number of S_e <= u = the largest e with S_e <= u
    L2, S2 = plan.L[e2 - 1], plan.S[e2 - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = np.where(L2 > 0.0, np.minimum((u - S2) / L2, 1.0), 0.0)
    p2, d2 = plan.at(e2, r2) if len(u) else (np.empty((0, 3)), np.empty(0, dtype=np.int64))
    c2 = cost(v, p2, w)
    # ---- the least of the stage-1 winner and the stage-2 candidates, the winner first among equals
    cc, ss = np.concatenate([c1[k1:k1 + 1], c2]), np.concatenate([arc[k1:k1 + 1], u])
    b = first_best(cc, ss)
    best_c, best_s = cc[b], ss[b]
    other = c2[u != best_s]
    far = c1[inside][np.abs(arc[inside] - best_s) > 2.0 * spacing]
    decided = bool((other > best_c + EPS).all() and (far > best_c + EPS).all())
    pick = (edge[k1], direction[k1], s1, ratio[k1], poses[k1]) if b == 0 else (e2[b - 1], d2[b - 1], u[b - 1], r2[b - 1], p2[b - 1])
    return record(*pick, int(keep.sum()), decided, lambda edge, ratio: float(cost(v, plan.at([edge], [ratio])[0], w)[0]))


OUTSIDE = 40.0  # metres beyond the map's edge


def vehicle_poses(plan, start, goal, half, rng, n_random=5):
    """[n_random + 3, 3] vehicle poses for one plan: points of the plan at arbitrary s pushed sideways by up to 0.5 m and turned by up to 0.3 rad, the
    exact start pose, the exact goal pose, a pose 40 m outside a map of half-width `half`.  (No plan: the same around the start pose.)"""
    out = []
    for _ in range(n_random):
        u, side, turn = rng.uniform(0.0, 1.0), rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3)
        if plan is None or not plan.edges:
            x, y, t = start if plan is None else plan.first
        else:
            u = u * plan.length
            e = int(np.searchsorted(plan.S, u, side="right"))
            (x, y, t), = plan.at([e], [min((u - plan.S[e - 1]) / plan.L[e - 1], 1.0) if plan.L[e - 1] > 0 else 0.0])[0]
        out.append((x - side * math.sin(t), y + side * math.cos(t), t + turn))
    out += [tuple(start), tuple(goal), (half + OUTSIDE, rng.uniform(-half, half), rng.uniform(-3.1, 3.1))]
    return np.array(out, dtype=np.float64)
