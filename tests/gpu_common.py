"""Shared helpers for the -m gpu parity tests: an oracle World and the matching device map set."""
import math

import numpy as np

import oracle_lib as O


def make_pair(n_cells, n_obstacles, seed, resolution=0.1, ctx=None):
    """Returns (oracle world, device map set, validator) over identical grids."""
    import pathplanning_amd as pa
    w = O.synthetic_world(n_cells, n_obstacles, seed, resolution)
    ctx = ctx or pa.Context(0)
    ms = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, resolution)
    assert (ms.rows, ms.cols) == (w.rows, w.cols)
    assert np.allclose(ms.grid_origin, w.origin, rtol=0, atol=0)
    ms.upload_dist2(w.d2())
    ms.upload_occupancy(w.occ())
    ms.upload_path_cost(w.pathcost())
    val = pa.StateValidatorOccupancyMap(ms)
    return w, ms, val, ctx


def make_pair_bounds(lower, upper, resolution, n_obstacles, seed, ctx=None):
    """make_pair over any state box and cell size (oracle_lib.synthetic_world's bounds form): (oracle world, device map set, validator,
    context), device dims and grid origin asserted equal to the oracle's."""
    import pathplanning_amd as pa
    w = O.synthetic_world(0, n_obstacles, seed, resolution, lower=lower, upper=upper)
    ctx = ctx or pa.Context(0)
    ms = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, resolution)
    assert (ms.rows, ms.cols) == (w.rows, w.cols)
    assert np.allclose(ms.grid_origin, w.origin, rtol=0, atol=0)
    ms.upload_dist2(w.d2())
    ms.upload_occupancy(w.occ())
    ms.upload_path_cost(w.pathcost())
    val = pa.StateValidatorOccupancyMap(ms)
    return w, ms, val, ctx


def box_random_poses(rng, w, n, margin=0.05):
    """uniform poses over the union of the state box and the grid's extent, widened by `margin` of that extent on every side;
    headings over +-1.2 pi"""
    lo = np.minimum(w.lb[:2], w.grid_lo)
    hi = np.maximum(w.ub[:2], w.grid_hi)
    pad = margin * (hi - lo)
    p = np.empty((n, 3))
    p[:, 0] = rng.uniform(lo[0] - pad[0], hi[0] + pad[0], n)
    p[:, 1] = rng.uniform(lo[1] - pad[1], hi[1] + pad[1], n)
    p[:, 2] = rng.uniform(-1.2 * math.pi, 1.2 * math.pi, n)
    return p


def box_valid_random_poses(rng, w, n):
    """valid poses (the oracle's verdict), headings in [-pi, pi], on any box"""
    out = []
    while len(out) < n:
        p = box_random_poses(rng, w, 4 * n, margin=0.0)
        p[:, 2] = rng.uniform(-math.pi, math.pi, len(p))
        ok = w.is_state_valid(p).astype(bool)
        out.extend(list(p[ok]))
    return np.array(out[:n])


def random_poses(rng, w, n, margin=1.05):
    half = w.ub[0]
    p = np.empty((n, 3))
    p[:, 0] = rng.uniform(-margin * half, margin * half, n)
    p[:, 1] = rng.uniform(-margin * half, margin * half, n)
    p[:, 2] = rng.uniform(-1.2 * math.pi, 1.2 * math.pi, n)
    return p


def valid_random_poses(rng, w, n):
    out = []
    while len(out) < n:
        p = random_poses(rng, w, 4 * n, margin=0.98)
        p[:, 2] = rng.uniform(-math.pi, math.pi, len(p))
        ok = w.is_state_valid(p).astype(bool)
        out.extend(list(p[ok]))
    return np.array(out[:n])


# ------------------------------------------------------------------------------------------ outlines on any box --
def rect_vertices(dx, dy):
    return [(dx / 2.0, dy / 2.0), (-dx / 2.0, dy / 2.0), (-dx / 2.0, -dy / 2.0), (dx / 2.0, -dy / 2.0)]  # RectangleShape, obstacle.cpp:106-110


def circle_vertices(radius, count):
    radius *= 1.0 / math.cos(math.pi / count)  # CircleShape, obstacle.cpp:112-122 (the angle goes through a float division)
    return [(radius * math.cos(2 * math.pi * i / float(np.float32(count))), radius * math.sin(2 * math.pi * i / float(np.float32(count)))) for i in range(count)]


def build_pair_bounds(lower, upper, resolution, shapes, ctx=None):
    """The same outlines in an oracle world over any state box and cell size (World.add_rectangle / add_circle: AddObstacle) and on
    the device (host vertices, device Bresenham), obstacle k with id k.  shapes: ("rect", dx, dy, pose) or ("circle", radius, count,
    pose).  Returns (oracle world, device map set, context); the world's brushfire is not run (w.update())."""
    import pathplanning_amd as pa
    w = O.World(lower=lower, upper=upper, resolution=resolution)
    ctx = ctx or pa.Context(0)
    ms = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, resolution)
    assert (ms.rows, ms.cols) == (w.rows, w.cols)
    assert np.array_equal(ms.grid_origin, w.origin)
    for k, (kind, a, b, pose) in enumerate(shapes):
        if kind == "rect":
            assert w.add_rectangle(a, b, pose) == k
            ms.add_polygon(rect_vertices(a, b), pose, k)
        else:
            assert w.add_circle(a, b, pose) == k
            ms.add_polygon(circle_vertices(a, b), pose, k)
    return w, ms, ctx


# ------------------------------------------------------- plain numpy restatements of the exact-transform fields --
INT_MAX = 2**31 - 1
NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def exact_sq_edt(sources):
    """Exact squared Euclidean distance (int64) of every cell to the nearest True cell of `sources`, INT_MAX everywhere when there is
    none; from scipy's exact transform, through its nearest-feature indices, so the values are integers computed here."""
    from scipy import ndimage
    if not sources.any():
        return np.full(sources.shape, INT_MAX, np.int64)
    _, (ir, ic) = ndimage.distance_transform_edt(~sources, return_indices=True)
    rr, cc = np.indices(sources.shape)
    return (ir.astype(np.int64) - rr) ** 2 + (ic.astype(np.int64) - cc) ** 2


def brute_sq_edt(sources, chunk=2048):
    """exact_sq_edt by brute force over every source cell (small grids)"""
    src = np.argwhere(sources).astype(np.int64)
    out = np.full(sources.size, INT_MAX, np.int64)
    if len(src) == 0:
        return out.reshape(sources.shape)
    cells = np.indices(sources.shape).reshape(2, -1).T.astype(np.int64)
    for i in range(0, len(cells), chunk):
        c = cells[i:i + chunk]
        out[i:i + chunk] = (((c[:, None, :] - src[None, :, :]) ** 2).sum(-1)).min(1)
    return out.reshape(sources.shape)


def labels_are_nearest(sources, d2, labels):
    """every label is a source cell at exactly squared distance d2 from its cell; (-1, -1) exactly where d2 is INT_MAX (no source)"""
    lr, lc = labels[..., 0].astype(np.int64), labels[..., 1].astype(np.int64)
    none = d2 == INT_MAX
    if not np.array_equal(none, lr < 0) or not np.array_equal(none, lc < 0):
        return False
    rr, cc = np.indices(d2.shape)
    ok = ~none
    rows, cols = d2.shape
    if (lr[ok] >= rows).any() or (lc[ok] >= cols).any():
        return False
    return bool(sources[lr[ok], lc[ok]].all() and np.array_equal((lr[ok] - rr[ok]) ** 2 + (lc[ok] - cc[ok]) ** 2, d2[ok].astype(np.int64)))


def check_voro(labels, occ):
    """CheckVoro (gvd.cpp:105-131) applied to fixed nearest-obstacle labels, every cell s against each of its 8 neighbours n, in the
    reference's order: nothing when both labels carry the same obstacle id; nothing unless d(s) > 1 or d(n) > 1; nothing when the two
    labels are the same or adjacent cells; nothing when either stability (the distance to the other side's label minus the own
    distance) is negative; then s is marked when its stability is <= n's (and n when n's is <= s's: the pair seen from n).  Labels
    (-1, -1) (no obstacle) mark nothing.  Returns the bool edge grid."""
    rows, cols = occ.shape
    lr, lc = labels[..., 0].astype(np.int64), labels[..., 1].astype(np.int64)
    valid = lr >= 0
    rr, cc = np.indices((rows, cols))
    ident = np.where(valid, occ[np.where(valid, lr, 0), np.where(valid, lc, 0)], -2)
    d = (lr - rr) ** 2 + (lc - cc) ** 2
    mark = np.zeros((rows, cols), bool)
    for dr, dc in NEIGHBOURS:
        s = (slice(max(0, -dr), rows - max(0, dr)), slice(max(0, -dc), cols - max(0, dc)))  # cells whose neighbour is in the grid
        n = (slice(max(0, dr), rows - max(0, -dr)), slice(max(0, dc), cols - max(0, -dc)))
        ok = valid[s] & valid[n] & (ident[s] != ident[n])
        ok &= (d[s] > 1) | (d[n] > 1)
        ok &= (np.abs(lr[s] - lr[n]) > 1) | (np.abs(lc[s] - lc[n]) > 1)
        s_stab = (lr[n] - rr[s]) ** 2 + (lc[n] - cc[s]) ** 2 - d[s]
        n_stab = (lr[s] - rr[n]) ** 2 + (lc[s] - cc[n]) ** 2 - d[n]
        ok &= (s_stab >= 0) & (n_stab >= 0) & (s_stab <= n_stab)
        mark[s] |= ok
    return mark


def path_cost(d2, voronoi_d2, resolution, alpha=20.0, d_max=30.0):
    """PathCostMap::Update (gvd.cpp:266-283) with the reference's types: the distances are float(sqrt(int) * resolution) (gvd.h:38,
    :78), the two quotients and their product are float, pow(float, 2) and the last quotient double, the store float; zero where
    the obstacle distance reaches d_max (or the Voronoi distance is infinite)."""
    res = np.float64(np.float32(resolution))
    od = (np.sqrt(np.asarray(d2, np.float64)) * res).astype(np.float32)
    vd = (np.sqrt(np.asarray(voronoi_d2, np.float64)) * res).astype(np.float32)
    a, dm = np.float32(alpha), np.float32(d_max)
    with np.errstate(divide="ignore", invalid="ignore"):
        ab = (a / (a + od)) * (vd / (od + vd))  # float32 throughout
        x = (od - dm).astype(np.float64)
        val = (ab.astype(np.float64) * ((x * x) / (np.float64(dm) * np.float64(dm)))).astype(np.float32)
    return np.where((od >= dm) | np.isinf(vd), np.float32(0.0), val)
