"""Numpy restatement of the vehicle-footprint checks (include/pp_hip.h, "vehicle footprint"): the yardstick of
tests/test_footprint_host.py and tests/test_gpu_footprint.py.  Worlds are oracle_lib.World objects whose local origin is (0, 0).

Every function also reports, per case, whether any sample had the reference point or a disc centre within GUARD cells of a
cell boundary (the project's guard band): there a last-bit difference between the device's and numpy's sin / cos
may pick another cell, and the case is left out of exact comparison.  At most MAX_LEFT_OUT of the cases of a test may be."""
import math

import numpy as np

import oracle_lib as O

GUARD = 1e-9
MAX_LEFT_OUT = 1e-3
F32 = np.float32

CAR3 = [(-0.2, 0.0, 1.3), (1.4, 0.0, 1.3), (3.0, 0.0, 1.3)]
TWO_RADII = [(0.0, 0.0, 0.9), (2.5, 0.4, 0.6), (2.5, -0.4, 0.6)]


class Grid:
    """what the checks read of a world: bounds, grid geometry, float distance grid (gvd.h:38)"""

    def __init__(self, w, d2=None, min_interp=0.1):
        self.lb, self.ub = w.lb, w.ub
        self.rows, self.cols = w.rows, w.cols
        self.origin = w.origin
        self.resd = np.float64(w.resolution)
        d2 = w.d2() if d2 is None else d2
        self.dist = (np.sqrt(d2.astype(np.float64)) * self.resd).astype(F32)
        self.min_interp = F32(min_interp)


def cover_rectangle(length, width, rear_overhang, n):
    """pp_footprint_cover_rectangle: n equal discs on the long axis, radius rounded UP to float"""
    s = length / n
    rd = math.sqrt((s / 2) * (s / 2) + (width / 2) * (width / 2))
    r = F32(rd)
    if float(r) < rd:
        r = np.nextafter(r, F32(np.inf))
    return [(-rear_overhang + (i + 0.5) * s, 0.0, float(r)) for i in range(n)]


def rho_of(discs):
    return max(math.hypot(ox, oy) for ox, oy, _ in discs)


def wrap(t):
    t = np.array(t, dtype=np.float64, copy=True)
    for _ in range(64):
        hi, lo = t > math.pi, t < -math.pi
        if not (hi.any() or lo.any()):
            break
        t = np.where(hi, t - 2 * math.pi, np.where(lo, t + 2 * math.pi, t))
    return t


def cell(g, x, y):
    """WorldPositionToGridCell(bounded = false): trunc((v - origin) / resolution); non-finite -> far outside"""
    with np.errstate(invalid="ignore"):
        qx, qy = (x - g.origin[0]) / g.resd, (y - g.origin[1]) / g.resd
        r = np.where(np.abs(qx) < 2.0e9, np.trunc(qx), -1.0).astype(np.int64)
        c = np.where(np.abs(qy) < 2.0e9, np.trunc(qy), -1.0).astype(np.int64)
    return r, c, qx, qy


def near_boundary(qx, qy):
    with np.errstate(invalid="ignore"):
        return (np.abs(qx - np.rint(qx)) < GUARD) | (np.abs(qy - np.rint(qy)) < GUARD)


def fp_state(g, p, discs):
    """-> valid, clearance (f32, meaningful where valid), border (f32, same), guard"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    x, y, t = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):
        ok = (x >= g.lb[0]) & (x <= g.ub[0]) & (y >= g.lb[1]) & (y <= g.ub[1])
        lt = wrap(t)
        ok &= (lt >= g.lb[2]) & (lt <= g.ub[2])
        r, c, qx, qy = cell(g, x, y)
        ok &= (r >= 0) & (r < g.rows) & (c >= 0) & (c < g.cols)
        guard = near_boundary(qx, qy)
        clear = np.full(len(p), np.inf, F32)
        border = np.minimum.reduce([x - g.lb[0], g.ub[0] - x, y - g.lb[1], g.ub[1] - y])
        ct, st = np.cos(t), np.sin(t)
        for ox, oy, rad in discs:
            cx, cy = (x, y) if ox == 0 and oy == 0 else ((x + ox * ct) - oy * st, (y + ox * st) + oy * ct)
            inb = (cx >= g.lb[0]) & (cx <= g.ub[0]) & (cy >= g.lb[1]) & (cy <= g.ub[1])
            r, c, qx, qy = cell(g, cx, cy)
            guard |= near_boundary(qx, qy)
            ins = inb & (r >= 0) & (r < g.rows) & (c >= 0) & (c < g.cols)
            d = np.where(ins, g.dist[np.clip(r, 0, g.rows - 1), np.clip(c, 0, g.cols - 1)], F32(-1))
            ok &= ins & (d >= F32(rad))
            clear = np.minimum(clear, (d - F32(rad)).astype(F32))
            border = np.minimum(border, np.minimum.reduce([cx - g.lb[0], g.ub[0] - cx, cy - g.lb[1], g.ub[1] - cy]))
    return ok, clear, border.astype(F32), guard


def march(g, discs, init, length, gain, interp):
    """The march of IsPathValid over a footprint.  interp(idx, ratio) -> poses of paths idx at the given ratios.
    -> valid, last (f32), guard, samples per path"""
    n = len(length)
    length = np.asarray(length, dtype=np.float64)
    gain = np.asarray(gain, dtype=F32)
    L, lastv = np.zeros(n), np.zeros(n)
    done, valid, guard = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    samples = np.zeros(n, np.int64)
    zero = length == 0.0
    if zero.any():
        ok, _, _, gd = fp_state(g, np.asarray(init)[zero], discs)
        valid[zero], guard[zero], done[zero] = ok, gd, True
    skip = ~zero & ~(0.0 < length)  # the loop is never entered
    valid[skip], done[skip] = True, True
    while not done.all():
        idx = np.nonzero(~done)[0]
        s = interp(idx, L[idx] / length[idx])
        ok, clear, border, gd = fp_state(g, s, discs)
        samples[idx] += 1
        guard[idx] |= gd
        done[idx[~ok]] = True
        ci = idx[ok]
        lastv[ci] = L[ci]
        step = np.maximum((np.minimum(clear[ok], border[ok]) / gain[ci]).astype(F32), g.min_interp).astype(F32)
        L[ci] = L[ci] + step.astype(np.float64)
        fin = ci[~(L[ci] < length[ci])]
        valid[fin], done[fin] = True, True
    with np.errstate(invalid="ignore", divide="ignore"):
        last = np.where(valid | zero, F32(1.0), (lastv / length).astype(F32)).astype(F32)
    return valid, last, guard, samples


def constant_steer(frm, kappa, d):
    """KinematicBicycleModel::ConstantSteer with rearToCenter = 0 (kinematic_bicycle_model.cpp:5-32); theta not wrapped"""
    frm = np.asarray(frm, dtype=np.float64).reshape(-1, 3)
    x, y, t = frm[:, 0], frm[:, 1], frm[:, 2]
    turn = np.abs(kappa) > 1e-9
    ks = np.where(turn, kappa, 1.0)
    t2 = np.where(turn, t + d * kappa, t)
    x2 = np.where(turn, x + 1 / ks * (np.sin(t2) - np.sin(t)), x + d * np.cos(t))
    y2 = np.where(turn, y + 1 / ks * (-np.cos(t2) + np.cos(t)), y + d * np.sin(t))
    return np.column_stack([x2, y2, t2])


def fp_arcs(g, frm, kappa, length, backward, discs):
    """constant-steer arcs (PathConstantSteer::Interpolate: distance = length * ratio, negated backwards) -> valid, last, guard, samples"""
    frm = np.asarray(frm, dtype=np.float64).reshape(-1, 3)
    n = len(frm)
    kappa = np.ascontiguousarray(np.broadcast_to(np.asarray(kappa, dtype=np.float64), n))
    length = np.ascontiguousarray(np.broadcast_to(np.asarray(length, dtype=np.float64), n))
    sign = np.where(np.broadcast_to(np.asarray(backward), n) != 0, -1.0, 1.0)
    gain = (1.0 + np.abs(kappa) * rho_of(discs)).astype(F32)

    def interp(idx, ratio):
        return constant_steer(frm[idx], kappa[idx], sign[idx] * (length[idx] * ratio))

    return march(g, discs, frm, length, gain, interp)


def fp_rs_paths(g, paths, discs):
    """Reeds-Shepp paths (records of oracle_lib.RS_PATH_DTYPE), samples from the oracle's PathReedsShepp::Interpolate"""
    p = np.ascontiguousarray(paths, dtype=O.RS_PATH_DTYPE).reshape(-1)
    gain = (1.0 + (1.0 / p["min_turning_radius"]) * rho_of(discs)).astype(F32)

    def interp(idx, ratio):
        return O.rs_path_interpolate(p[idx], ratio)[0]

    return march(g, discs, p["start"], p["length"], gain, interp)


def fp_se2_paths(g, start, end, discs):
    """PathSE2 (paths/path_se2.cpp): headings wrapped on construction, everything interpolated linearly"""
    a = np.array(start, dtype=np.float64).reshape(-1, 3)
    b = np.array(end, dtype=np.float64).reshape(-1, 3)
    a[:, 2], b[:, 2] = wrap(a[:, 2]), wrap(b[:, 2])
    length = np.sqrt((b[:, 0] - a[:, 0]) * (b[:, 0] - a[:, 0]) + (b[:, 1] - a[:, 1]) * (b[:, 1] - a[:, 1]))
    with np.errstate(invalid="ignore", divide="ignore"):
        gain = np.where(length == 0.0, 1.0, 1.0 + (np.abs(b[:, 2] - a[:, 2]) / length) * rho_of(discs)).astype(F32)

    def interp(idx, ratio):
        r = ratio[:, None]
        return (1 - r) * a[idx] + r * b[idx]

    return march(g, discs, a, length, gain, interp)


def continuous_poses(rng, w, n, margin=1.05):
    """continuous random poses (never on multiples of the resolution) over the state box widened by `margin`; headings over +-1.2 pi"""
    p = np.empty((n, 3))
    p[:, 0] = rng.uniform(margin * w.lb[0], margin * w.ub[0], n)
    p[:, 1] = rng.uniform(margin * w.lb[1], margin * w.ub[1], n)
    p[:, 2] = rng.uniform(-1.2 * math.pi, 1.2 * math.pi, n)
    return p


def valid_poses(rng, g, w, n, discs):
    """poses valid for the footprint (this restatement), headings in [-pi, pi]"""
    out = []
    while len(out) < n:
        p = continuous_poses(rng, w, 4 * n, margin=0.98)
        p[:, 2] = rng.uniform(-math.pi, math.pi, len(p))
        out.extend(list(p[fp_state(g, p, discs)[0]]))
    return np.array(out[:n])
