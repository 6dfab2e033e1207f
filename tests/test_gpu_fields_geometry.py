"""-m gpu: outlines -> occupancy -> GVD fields -> post-processing off the default geometry, and the exact-transform field mode against
its own definition.

tests/test_gpu_gvd.py and tests/test_gpu_postprocess.py build every map as a square of 0.1 m cells centred on the origin, where swapped
rows and columns, a mixed-up grid origin or a wrong cell size in the rasteriser, the two transform passes, the Voronoi rule, the path
cost or the smoother's label-to-world conversion go unnoticed.  Here: the four worlds of tests/test_gpu_geometry.py (non-square, 0.05 m
and 0.15 m cells, an off-centre state box) built from rectangle and circle outlines, plus E (96 x 1100 cells: rows of five 256-column
tiles of k_edt_rows, with rows whose only source is in the first or in the last tile) and F (1100 x 96 cells: long walks of k_edt_cols).
Each world asserts the property it exists for before anything is compared.

The exact-transform mode (PP_GVD_EXACT_EDT, what pp_map_update_gvd runs) is fully defined once its own obstacle labels are fixed, so it
is compared exactly with the numpy restatements of tests/gpu_common.py (checked against the oracle by tests/test_field_restatements.py):
the exact squared transform, CheckVoro on the device's labels, the transform of that edge set, and PathCostMap::Update at any
alpha / d_max."""
import math

import numpy as np
import pytest

import oracle_lib as O
from scipy import ndimage

from gpu_common import (INT_MAX, box_valid_random_poses, brute_sq_edt, build_pair_bounds, check_voro, exact_sq_edt, labels_are_nearest, path_cost,
                        rect_vertices)
from test_gpu_geometry import PARAMS, WORLDS, env
from test_gpu_grid_astar import random_free_cells, same
from test_gpu_gvd import assert_fields_equal_the_brushfire, build_pair, seeded_shapes
from test_gpu_hybrid import compare, run_pair
from test_gpu_postprocess import run

pytestmark = pytest.mark.gpu

TILE = 256  # k_edt_rows walks a row in tiles of this many columns

FIELD_WORLDS = {name: dict(lower=s["lower"], upper=s["upper"], res=s["res"], dims=s["dims"], seed=s["seed"], obstacles=s["obstacles"]) for name, s in WORLDS.items()}
# wide and short: columns span five tiles of the row pass; random outlines in a band of rows, two small circles outside it in the
# first and in the last tile
FIELD_WORLDS["E"] = dict(lower=(-4.8, -55.0), upper=(4.8, 55.0), res=0.1, dims=(96, 1100), seed=5, obstacles=8)
# tall and narrow: the column pass walks hundreds of rows between the band of outlines and the two circles far above and below it
FIELD_WORLDS["F"] = dict(lower=(-55.0, -4.8), upper=(55.0, 4.8), res=0.1, dims=(1100, 96), seed=6, obstacles=8)

# (alpha, d_max) pairs of PathCostMap: the reference's, one whose small d_max zeroes most cells, one in between
COST_PAIRS = [(20.0, 30.0), (5.0, 1.5), (60.0, 8.0)]


def field_geometry(name):
    """(grid_lo, grid_hi) of a world's grid, from the oracle's sizing"""
    spec = FIELD_WORLDS[name]
    w = O.World(lower=spec["lower"], upper=spec["upper"], resolution=spec["res"])
    return w.grid_lo.copy(), w.grid_hi.copy()


def field_shapes(name):
    """The outlines of a world, ("rect", dx, dy, pose) / ("circle", radius, vertices, pose), obstacle k gets id k: seeded rectangles and
    circles, one rectangle across the grid's upper column border, one circle over its lower corner; world D adds one rectangle inside
    the box but off the grid, one across the grid's upper row border inside the box and one on the grid but outside the box; E and F
    add the two far circles."""
    spec = FIELD_WORLDS[name]
    lo, hi = field_geometry(name)
    hx, hy = (hi - lo) / 2.0
    mid = (hi + lo) / 2.0
    half = min(hx, hy)
    band = {"E": (0.3 * hx, 0.35 * hy), "F": (0.35 * hx, 0.3 * hy)}.get(name, (0.7 * hx, 0.7 * hy))
    rng = np.random.RandomState(100 + spec["seed"])
    out = []
    for k in range(spec["obstacles"]):
        x, y = mid[0] + rng.uniform(-band[0], band[0]), mid[1] + rng.uniform(-band[1], band[1])
        th = rng.uniform(-math.pi, math.pi)
        out.append(("circle", 0.08 * half, 10, [x, y, th]) if k % 3 == 0 else ("rect", 0.3 * half, 0.04 * half, [x, y, th]))
    out.append(("rect", 0.6, 1.5, [mid[0], hi[1] - 0.2, 0.0]))  # across the last column
    out.append(("circle", 0.8, 12, [lo[0] + 0.1, lo[1] + 0.1, 0.2]))  # over the (0, 0) corner
    if name == "D":
        out.append(("rect", 2.0, 1.0, [16.0, -5.0, 0.3]))  # inside the box, off the grid (grid x < 13.1)
        out.append(("rect", 1.5, 0.5, [13.0, -8.0, 0.0]))  # across the last row, inside the box
        out.append(("rect", 1.0, 1.0, [0.0, 8.0, 0.0]))  # on the grid, outside the box (box y <= 4.4)
    if name == "E":
        out.append(("circle", 0.3, 8, [lo[0] + 0.9, lo[1] + 23.5, 0.0]))  # rows ~9, columns ~235: first tile
        out.append(("circle", 0.3, 8, [hi[0] - 0.9, hi[1] - 3.0, 0.0]))  # rows ~87, columns ~1070: last tile
    if name == "F":
        out.append(("circle", 0.3, 8, [lo[0] + 3.0, lo[1] + 2.0, 0.0]))  # rows ~30
        out.append(("circle", 0.3, 8, [hi[0] - 3.0, hi[1] - 2.0, 0.0]))  # rows ~1070
    return out


def field_pair(name, ctx=None):
    """a world's outlines in the oracle and on the device; the oracle's brushfire is run"""
    spec = FIELD_WORLDS[name]
    w, ms, ctx = build_pair_bounds(spec["lower"], spec["upper"], spec["res"], field_shapes(name), ctx)
    assert (w.rows, w.cols) == spec["dims"], (name, w.rows, w.cols)
    w.update()
    return w, ms, ctx


_PAIRS = {}


def shared_pair(name):
    """field_pair built once per module, for the tests that only read it"""
    if name not in _PAIRS:
        _PAIRS[name] = field_pair(name)
    return _PAIRS[name]


def rows_with_sources_only_in(occ, tile):
    """rows whose occupied cells all lie in column tile `tile` of the row pass (and which have some)"""
    cols = occ.shape[1]
    t0, t1 = tile * TILE, min(cols, (tile + 1) * TILE)
    src = occ >= 0
    inside = src[:, t0:t1].any(1)
    outside = src[:, :t0].any(1) | src[:, t1:].any(1)
    return np.nonzero(inside & ~outside)[0]


@pytest.mark.parametrize("name", list(FIELD_WORLDS))
def test_field_world_geometry(name):
    """the preconditions of every other test here"""
    w, ms, ctx = shared_pair(name)
    occ = w.occ()
    shapes = field_shapes(name)
    assert w.rows != w.cols
    assert 0.001 < (occ >= 0).mean() < 0.1
    ids = set(np.unique(occ[occ >= 0]).tolist())
    # the border-crossing outlines reach the last column and the (0, 0) corner, and are cut there
    k_edge, k_corner = FIELD_WORLDS[name]["obstacles"], FIELD_WORLDS[name]["obstacles"] + 1
    assert (occ[:, -1] == k_edge).any() and (occ[0, :] == k_corner).any() and (occ[:, 0] == k_corner).any()
    if name == "D":
        k_off, k_row_edge, k_outside_box = k_corner + 1, k_corner + 2, k_corner + 3
        x, y = shapes[k_off][3][:2]
        assert w.lb[0] < x < w.ub[0] and w.lb[1] < y < w.ub[1] and x - 1.2 > w.grid_hi[0]  # inside the box, wholly off the grid
        assert k_off not in ids  # nothing rasterised
        assert (occ[-1, :] == k_row_edge).any()
        x, y = shapes[k_outside_box][3][:2]
        assert w.ub[1] < y - 0.5 and y + 0.5 < w.grid_hi[1] and k_outside_box in ids  # on the grid, outside the box: rasterised
    if name == "E":
        tiles = (w.cols + TILE - 1) // TILE
        assert tiles == 5
        _, (ir, ic) = ndimage.distance_transform_edt(occ < 0, return_indices=True)
        cc = np.indices(occ.shape)[1]
        for tile in (0, tiles - 1):  # rows whose only sources lie in this tile, and cells of other tiles whose nearest source is there
            rows = rows_with_sources_only_in(occ, tile)
            reach = np.isin(ir, rows) & (ic // TILE != cc // TILE)
            assert len(rows) >= 3 and reach.sum() >= 100, (tile, rows, int(reach.sum()))
    if name == "F":
        d2 = exact_sq_edt(occ >= 0)
        _, (ir, _) = ndimage.distance_transform_edt(occ < 0, return_indices=True)
        walk = np.abs(ir - np.arange(w.rows)[:, None])
        assert walk.max() > 150 and (walk > 100).mean() > 0.1 and d2.max() > 150 ** 2


@pytest.mark.parametrize("name", list(FIELD_WORLDS))
def test_outline_rasterisation(name):
    """device occupancy = the oracle's AddObstacle, also after RemoveObstacle (-1 over the outline) of the border-crossing rectangle,
    on D of the off-grid one, and of a seeded one"""
    w, ms, ctx = field_pair(name)
    assert np.array_equal(ms.download_occupancy(), w.occ())
    shapes = field_shapes(name)
    k_edge = FIELD_WORLDS[name]["obstacles"]
    removed = [k_edge] + ([k_edge + 2] if name == "D" else []) + [next(k for k, s in enumerate(shapes) if s[0] == "rect")]  # + a seeded one
    for k in removed:
        _, dx, dy, pose = shapes[k]
        w.remove_rectangle(k, dx, dy, pose)
        ms.add_polygon(rect_vertices(dx, dy), pose, -1)
        assert np.array_equal(ms.download_occupancy(), w.occ()), (name, k)
    assert not (w.occ() == removed[0]).any()


@pytest.mark.parametrize("name", list(FIELD_WORLDS))
def test_reference_order_mode(name):
    """PP_GVD_REFERENCE_ORDER: every grid of download_gvd equals the brushfire bit for bit -- first build, then an added rectangle and the
    removal of a seeded one (incremental)"""
    w, ms, ctx = field_pair(name)
    ms.update_gvd(mode=ms.GVD_REFERENCE_ORDER)
    g = assert_fields_equal_the_brushfire(ms, w, (name, "first build"))
    assert (g["voronoi_edge"] != 0).sum() > w.rows
    lo, hi = w.grid_lo, w.grid_hi
    extra = (0.12 * (hi[0] - lo[0]), 0.02 * (hi[1] - lo[1]), [0.55 * lo[0] + 0.45 * hi[0], 0.6 * lo[1] + 0.4 * hi[1], 0.7])
    ident = w.add_rectangle(*extra)
    ms.add_polygon(rect_vertices(extra[0], extra[1]), extra[2], ident)
    w.update()
    ms.update_gvd(mode=ms.GVD_REFERENCE_ORDER)
    assert_fields_equal_the_brushfire(ms, w, (name, "after adding"))
    shapes = field_shapes(name)
    k = next(i for i, s in enumerate(shapes) if s[0] == "rect")
    w.remove_rectangle(k, shapes[k][1], shapes[k][2], shapes[k][3])
    ms.add_polygon(rect_vertices(shapes[k][1], shapes[k][2]), shapes[k][3], -1)
    w.update()
    ms.update_gvd(mode=ms.GVD_REFERENCE_ORDER)
    assert_fields_equal_the_brushfire(ms, w, (name, "after removing"))


def assert_exact_fields(ms, res, where, brute=False):
    """every grid of the exact-transform mode against its definition, at the (alpha, d_max) pairs of COST_PAIRS; returns the share
    of cells in PathCostMap's zero branch (obstacle distance >= d_max) per pair"""
    occ = ms.download_occupancy()
    src = occ >= 0
    zero = []
    for alpha, d_max in COST_PAIRS:
        ms.update_gvd(alpha=alpha, d_max=d_max, mode=ms.GVD_EXACT_EDT)
        g = ms.download_gvd()
        if alpha == COST_PAIRS[0][0]:
            d2 = g["d2"].astype(np.int64)
            assert np.array_equal(d2, exact_sq_edt(src)), where
            if brute:
                assert np.array_equal(d2, brute_sq_edt(src)), where
            assert labels_are_nearest(src, d2, g["nearest_obstacle"]), where
            edge = g["voronoi_edge"] != 0
            assert np.array_equal(edge, check_voro(g["nearest_obstacle"], occ)), (where, int((edge != check_voro(g["nearest_obstacle"], occ)).sum()))
            vd2 = g["voronoi_d2"].astype(np.int64)
            assert np.array_equal(vd2, exact_sq_edt(edge)), where
            assert labels_are_nearest(edge, vd2, g["nearest_edge"]), where
            first = g
        else:  # the transforms do not depend on the pair
            for key in ("d2", "nearest_obstacle", "voronoi_edge", "voronoi_d2", "nearest_edge"):
                assert np.array_equal(g[key], first[key]), (where, key)
        want = path_cost(g["d2"], g["voronoi_d2"], res, alpha, d_max)
        assert np.array_equal(g["path_cost"].view(np.uint32), want.view(np.uint32)), (where, alpha, d_max)
        od = (np.sqrt(g["d2"].astype(np.float64)) * np.float64(np.float32(res))).astype(np.float32)
        zero.append(float((od >= np.float32(d_max)).mean()))
    return first, zero


@pytest.mark.parametrize("name", list(FIELD_WORLDS))
def test_exact_transform_mode_off_the_default_geometry(name):
    w, ms, ctx = shared_pair(name)
    g, zero = assert_exact_fields(ms, FIELD_WORLDS[name]["res"], name, brute=name == "C")
    assert (g["voronoi_edge"] != 0).sum() > w.rows
    assert zero[0] < 0.5 and 0.25 < zero[1] < 0.99, zero  # d_max = 1.5 m: a real share of the cells in the zero branch


@pytest.mark.parametrize("cells,n,seed", [(256, 6, 3), (512, 12, 1), (1024, 24, 1)])
def test_exact_transform_mode_on_square_maps(cells, n, seed):
    w, ms, ctx = build_pair(cells, seeded_shapes(cells, n, seed))
    g, zero = assert_exact_fields(ms, 0.1, cells)
    assert 0.25 < zero[1] < 0.99, zero


def test_exact_transform_mode_degenerate_maps():
    """no obstacle at all; a single obstacle id (no Voronoi edge anywhere); one obstacle cell in a corner"""
    import pathplanning_amd as pa
    ctx = pa.Context(0)
    lower, upper, res = FIELD_WORLDS["A"]["lower"], FIELD_WORLDS["A"]["upper"], FIELD_WORLDS["A"]["res"]
    box = O.World(lower=lower, upper=upper, resolution=res)
    ms = pa.OccupancyMapSet.from_bounds(ctx, box.lb, box.ub, res)
    rows, cols = ms.rows, ms.cols
    ms.upload_occupancy(np.full((rows, cols), -1, np.int32))
    g, _ = assert_exact_fields(ms, res, "obstacle-free")
    assert (g["d2"] == INT_MAX).all() and (g["nearest_obstacle"] == -1).all() and not g["voronoi_edge"].any()
    assert (g["voronoi_d2"] == INT_MAX).all() and (g["nearest_edge"] == -1).all() and (g["path_cost"] == 0).all()
    # one rectangle: one id, so no pair of labels can differ in it
    w, ms1, _ = build_pair_bounds(lower, upper, res, [("rect", 6.0, 0.8, [1.0, -2.0, 0.4])], ctx)
    g, _ = assert_exact_fields(ms1, res, "one id")
    assert (g["d2"] == 0).sum() > 50 and not g["voronoi_edge"].any() and (g["voronoi_d2"] == INT_MAX).all()
    # one cell in the last row's first column
    occ = np.full((rows, cols), -1, np.int32)
    occ[rows - 1, 0] = 3
    ms.upload_occupancy(occ)
    g, _ = assert_exact_fields(ms, res, "corner cell")
    assert g["d2"][0, cols - 1] == (rows - 1) ** 2 + (cols - 1) ** 2 and (g["nearest_obstacle"] == [rows - 1, 0]).all()
    assert not g["voronoi_edge"].any()


# (Not P4: its 0.7 forward multiplier makes ProcessPossibleShortcut compare totals of two paths to one pose that are equal in exact
# arithmetic, so the last bit of a device sin / cos against glibc's can decide whether a replacement node is created.  On A and D one
# query of 24 differs from the oracle in its node count alone, on the brushfire's own fields as much as on these.)
@pytest.mark.parametrize("wn,pn", [("A", "P1"), ("B", "P0"), ("D", "P0")])
def test_planning_on_exact_transform_fields(wn, pn):
    """The oracle reads the device's exact-transform grids (occupancy, d2, path cost): every query is identical -- status, expansion
    sequence, counters, cost, path -- and so are the validator's verdicts"""
    import pathplanning_amd as pa
    w, ms, ctx = field_pair(wn)
    ms.update_gvd(mode=ms.GVD_EXACT_EDT)
    g = ms.download_gvd()
    w.set_occ(ms.download_occupancy())
    w.set_d2(g["d2"])
    w.set_pathcost(g["path_cost"])
    val = pa.StateValidatorOccupancyMap(ms)
    rng = np.random.RandomState(300 + ord(wn))
    poses = np.concatenate([box_valid_random_poses(rng, w, 2000), np.column_stack([rng.uniform(w.grid_lo[0], w.grid_hi[0], 20000),
                                                                                 rng.uniform(w.grid_lo[1], w.grid_hi[1], 20000), rng.uniform(-3.2, 3.2, 20000)])])
    want = w.is_state_valid(poses).astype(bool)
    assert 0.05 < want.mean() < 0.98
    assert np.array_equal(val.is_state_valid(poses), want)
    n = 24
    starts, goals = box_valid_random_poses(rng, w, n), box_valid_random_poses(rng, w, n)
    seeds = np.arange(n, dtype=np.uint64) + 31
    planner, res, h = run_pair(w, ms, val, PARAMS[pn], starts, goals, seeds, max_nodes=131072)
    n_ok = compare(planner, res, h, starts, goals, seeds)
    planner.close()
    assert n_ok >= n // 3


def uploaded_labels_map(w, ctx):
    """a device map over the oracle's own brushfire grids (occupancy, d2, path cost, nearest cells uploaded)"""
    import pathplanning_amd as pa
    ms = pa.OccupancyMapSet.from_bounds(ctx, w.lb, w.ub, float(w.resolution))
    ms.upload_dist2(w.d2())
    ms.upload_occupancy(w.occ())
    ms.upload_path_cost(w.pathcost())
    ms.upload_nearest_cells(*O.world_nearest(w))
    return ms


def box_pairs(rng, w, n):
    return box_valid_random_poses(rng, w, n), box_valid_random_poses(rng, w, n)


POST_COMBOS = [(wn, pn) for wn in "ABCD" for pn in WORLDS[wn]["params"]]


@pytest.mark.parametrize("labels", ["uploaded", "device"])
@pytest.mark.parametrize("wn,pn", POST_COMBOS)
def test_postprocessing(wn, pn, labels):
    """Sampled path within 1e-9, cusp flags and point counts exact, status equal, smoothed path within 1e-5 (no escape clause) at 0.8 and
    0.5 m spacing and at 0.1 m with 10 iterations -- on labels uploaded from the oracle, and on the device's own reference-order fields"""
    import pathplanning_amd as pa
    w, ms0, ctx = shared_pair(wn)
    if labels == "uploaded":
        ms = uploaded_labels_map(w, ctx)
    else:
        ms = ms0
        ms.update_gvd(mode=ms.GVD_REFERENCE_ORDER)
        assert_fields_equal_the_brushfire(ms, w, wn)
    val = pa.StateValidatorOccupancyMap(ms)
    kw = PARAMS[pn]
    seed = 400 + ord(wn) + 7 * int(pn[1])
    n = 10
    for spacing, smoother in ((0.8, None), (0.5, dict(max_iterations=300, path_weight=0.1, voronoi_weight=0.05)), (0.1, dict(max_iterations=10))):
        s = run(w, ms, val, n, seed, spacing, smoother=smoother, costs=kw, strict_points=spacing == 0.1, pairs=box_pairs, upload_labels=False,
                max_nodes=131072)
        print("post-processing", wn, pn, labels, spacing, s)
        assert s["compared"] >= n // 3 and s["unstable_in_the_reference"] == 0, s


def short_pairs(rng, w, n):
    """valid starts with valid goals 0.3 .. 1.5 m away, headings within 0.4 rad: paths of fewer than 5 samples at 0.8 m"""
    starts = box_valid_random_poses(rng, w, 6 * n)
    goals = starts.copy()
    goals[:, :2] += rng.uniform(-1.5, 1.5, (len(goals), 2))
    goals[:, 2] = np.arctan2(np.sin(starts[:, 2] + rng.uniform(-0.4, 0.4, len(goals))), np.cos(starts[:, 2] + rng.uniform(-0.4, 0.4, len(goals))))
    ok = w.is_state_valid(goals).astype(bool) & (np.hypot(goals[:, 0] - starts[:, 0], goals[:, 1] - starts[:, 1]) > 0.3)
    assert ok.sum() >= n
    return starts[ok][:n], goals[ok][:n]


@pytest.mark.parametrize("wn", ["A", "D"])
def test_postprocessing_short_paths(wn):
    """paths of fewer than 5 samples: Smoother::Smooth only checks them (status 2, or -1 when a sample is invalid, smoother.cpp:45-50)"""
    import pathplanning_amd as pa
    w, ms0, ctx = shared_pair(wn)
    ms = uploaded_labels_map(w, ctx)
    val = pa.StateValidatorOccupancyMap(ms)
    s = run(w, ms, val, 16, 500 + ord(wn), 0.8, pairs=short_pairs, upload_labels=False)
    print("short paths", wn, s)
    assert s["short"] >= 6, s


def test_postprocessing_max_points_boundary():
    """max_points equal to a query's sample count: it passes; one below: that query (and every longer one) reports -4, whatever
    capacity an earlier call allocated"""
    import pathplanning_amd as pa
    w, ms0, ctx = shared_pair("A")
    ms = uploaded_labels_map(w, ctx)
    val = pa.StateValidatorOccupancyMap(ms)
    rng = np.random.RandomState(77)
    n = 12
    starts, goals = box_pairs(rng, w, n)
    seeds = np.arange(n, dtype=np.uint64) + 3
    planner = pa.HybridAStarBatch(val, pa.HybridAStarSearchParameters(), max_batch=n, max_nodes=32768)
    planner.initialize()
    res = planner.search_batch(starts, goals, seeds)
    h = O.Hybrid(w, table=planner.nonholo_table())
    spacing = 0.5
    want = []
    for q in range(n):
        r = h.search(starts[q], goals[q], int(seeds[q]))
        assert res[q].status == r["status"]
        want.append(O.postprocess(w, r, goals[q], O.params_array(), spacing) if r["status"] == 0 and len(r["path_poses"]) >= 2 else None)
    counts = sorted({x["n_points"] for x in want if x is not None})
    assert len(counts) >= 3 and counts[0] >= 9, counts
    first = planner.postprocess(path_interpolation=spacing)  # the default capacity (2048) is allocated first
    for k in (counts[len(counts) // 2], counts[-1]):
        for limit in (k, k - 1):
            post = planner.postprocess(path_interpolation=spacing, max_points=limit)
            for q in range(n):
                if want[q] is None:
                    continue
                if want[q]["n_points"] > limit:
                    assert post[q].smoothing_status == -4 and post[q].n_points == 0, (q, limit, want[q]["n_points"], post[q].smoothing_status)
                else:
                    assert post[q].n_points == want[q]["n_points"] and post[q].smoothing_status == first[q].smoothing_status, (q, limit)
                    g = planner.get_processed_path(q)
                    assert np.abs(g["sampled"] - want[q]["resampled"]).max() < 1e-9 and np.array_equal(g["cusp"], want[q]["cusp"])
    planner.close()


@pytest.mark.parametrize("name", list(WORLDS))
def test_grid_astar(name):
    """uni- and bidirectional grid A* on the non-square and off-centre grids: status, cost, path and expansion order identical"""
    import pathplanning_amd as pa
    w, ms, val, ctx = env(name)
    rng = np.random.RandomState(600 + ord(name))
    n = 24
    inits, goals = random_free_cells(w, rng, n), random_free_cells(w, rng, n)
    inits[0], goals[0] = (0, w.cols - 1), (w.rows - 1, 0)  # corner to corner: row and column bounds both reached
    g = pa.GridAStarBatch(ms)
    for bidirectional in (False, True):
        res = g.search_batch(inits, goals, bidirectional=bidirectional)
        n_ok = 0
        for q in range(n):
            want = O.grid_astar(w, inits[q], goals[q], bidirectional=bidirectional, inner_goal_f=goals[q], inner_goal_r=inits[q])
            same(res[q], want, bidirectional)
            n_ok += want["status"] == 0
        assert n_ok >= n // 2


@pytest.mark.parametrize("name", list(WORLDS))
def test_reeds_shepp_and_se2_path_validity(name):
    """IsPathValid over Reeds-Shepp paths at each turning radius the world is searched with, and over SE2 segments: bit-exact"""
    w, ms, val, ctx = env(name)
    rng = np.random.RandomState(700 + ord(name))
    n = 3000
    for pn in WORLDS[name]["params"]:
        rmin = {**O.DEFAULT_PARAMS, **PARAMS[pn]}["min_turning_radius"]
        a, b = box_valid_random_poses(rng, w, n), box_valid_random_poses(rng, w, n)
        b[: n // 2, :2] = a[: n // 2, :2] + rng.uniform(-4, 4, (n // 2, 2))
        P = O.rs_connect(a, b, rmin)
        P = np.concatenate([P, O.rs_path_truncate(P[:600], rng.uniform(0.1, 0.9, 600))])
        gv, gl = val.is_rs_path_valid(P)
        wv, wl = O.rs_paths_valid(w, P)
        assert np.array_equal(gv, wv) and np.array_equal(gl, wl), (name, pn)
        assert 0.05 < gv.mean() < 0.95
        gv, gl = val.is_se2_path_valid(a, b)
        wv, wl = O.se2_paths_valid(w, a, b)
        assert np.array_equal(gv, wv) and np.array_equal(gl, wl), (name, pn)
        assert 0.05 < gv.mean() < 0.95
