"""-m gpu: the rows kernels where their wave-uniform operands come from -- the expansion loop reads the map's bounds, origins, resolutions and
reciprocals, the heuristic's table geometry, the lattice and the key space from the kernel-argument segment, phase by phase (pp_rows_rs.hpp:
rows_kernargs_here), not from registers loaded once in front of the loop.  A wrong offset, a member read from the wrong argument or a load that
a branch skips would show as a different search, so all three instantiations that share the text run the same 64 queries against the CPU oracle:
  * k_hybrid_search_rows<true>: HybridAStarPipeline with 8 rows (every row is reclaimed several times),
  * k_hybrid_search_rows<false>: HybridAStarBatch with the rows kernel forced,
  * k_hybrid_search_rows_footprint<true>: the pipeline with the footprint {(0, 0, minSafeRadius)}, which is the point validator's search.
The map is 128 x 128 cells of 0.1 m with outline obstacles (arcs get truncated); eight queries run along the map's four borders (every bound is
compared against), two goals lie closer to an obstacle than the safe radius (the open list runs empty).  Status and every counter exact, cost
and path poses within 1e-5, no query left out."""
import math
import time

import numpy as np
import pytest

import oracle_lib as O
from gpu_common import make_pair, valid_random_poses

pytestmark = pytest.mark.gpu

N = 64
EXACT = ("status", "n_expanded", "n_state_checks", "n_path_checks", "n_rng_draws", "n_rs_attempts")
ARC = 1.5 * O.DEFAULT_PARAMS["spatial_resolution"]  # hybrid_a_star.cpp:115

_ENV = {}


def queries(w):
    rng = np.random.RandomState(103)
    starts, goals = valid_random_poses(rng, w, N), valid_random_poses(rng, w, N)
    cand = valid_random_poses(rng, w, 2000)
    k = 0
    for axis in (0, 1):  # from one border of the map to the opposite one, both ways, along x and along y
        for sign in (1, -1):
            order = np.argsort(sign * cand[:, axis])
            starts[k], goals[k] = cand[order[0]], cand[order[-1]]
            starts[k + 1], goals[k + 1] = cand[order[-2]], cand[order[1]]
            k += 2
    p = rng.uniform(-0.9 * w.ub[0], 0.9 * w.ub[0], (4000, 3))
    p[:, 2] = rng.uniform(-math.pi, math.pi, len(p))
    bad = p[~w.is_state_valid(p).astype(bool)]
    goals[k], goals[k + 1] = bad[0], bad[1]  # no valid path ends here
    return starts, goals, np.arange(N, dtype=np.uint64) + 500, k


def env():
    """world, device maps, the queries and the oracle's results (computed once, with the device's non-holonomic table)"""
    if not _ENV:
        import pathplanning_amd as pa
        w, ms, val, ctx = make_pair(128, 5, 3)
        starts, goals, seeds, n_border = queries(w)
        table, _ = pa.NonHolonomicHeuristic.build(ctx, w.lb, w.ub, pa.HybridAStarSearchParameters())
        h = O.Hybrid(w, O.params_array(), table=table)
        want = [h.search(starts[q], goals[q], int(seeds[q])) for q in range(N)]
        # the inputs reach what they are meant to reach (on the oracle): truncated arcs, Reeds-Shepp connections, failures, the map's borders
        solved = [r for r in want if r["status"] == 0]
        truncated = 0
        for r in solved:
            ch = h.children(r["path_poses"])  # every pose of a plan but the goal was expanded
            truncated += int(((ch["valid"] != 0) & (ch["length"] < ARC - 1e-9)).any())
        assert truncated >= 8 and sum(int((r["path_kind"] == 2).any()) for r in solved) >= 8 and N - len(solved) >= 2, (truncated, len(solved))
        assert want[n_border]["status"] != 0 and want[n_border + 1]["status"] != 0
        half, res = w.ub[0], float(w.resolution)
        for axis in (0, 1):
            edge = np.concatenate([starts[:n_border, axis], goals[:n_border, axis]])
            assert edge.max() > half - 8 * res and edge.min() < -half + 8 * res
        _ENV.update(w=w, ms=ms, val=val, ctx=ctx, starts=starts, goals=goals, seeds=seeds, table=table, want=want)
    return _ENV


def assert_is_the_oracles(q, got, poses, o):
    for f in EXACT:
        want = len(o["expanded"]) if f == "n_expanded" else o[f]
        assert getattr(got, f) == want, (q, f, getattr(got, f), want)
    if o["status"] == 0:
        assert abs(got.cost - o["cost"]) < 1e-5, (q, got.cost, o["cost"])
        assert len(poses) == len(o["path_poses"]) and np.abs(poses - o["path_poses"]).max() < 1e-5, q


def through_the_pipeline(E, footprint):
    import pathplanning_amd as pa
    pipe = pa.HybridAStarPipeline(E["val"], capacity=24, max_nodes=32768, search_rows=8)  # 64 queries over 8 rows and 24 field slots
    pipe.initialize(E["table"])
    if footprint:
        pipe.set_footprint(pa.Footprint(E["ms"], [(0.0, 0.0, E["val"].min_safe_radius)]))
    index_of, nxt, seen = {}, 0, set()
    t0 = time.time()
    while len(seen) < N:
        if nxt < N and pipe.free_slots() > 0:
            k = min(N - nxt, 13)
            for i, t in enumerate(pipe.submit(E["starts"][nxt:nxt + k], E["goals"][nxt:nxt + k], E["seeds"][nxt:nxt + k])):
                index_of[int(t)] = nxt + i
            nxt = len(index_of)
        tickets, res = pipe.poll(64, release=False)
        for i, t in enumerate(tickets):
            q = index_of[int(t)]
            assert_is_the_oracles(q, res[i], pipe.get_path_of(int(t))["poses"] if res[i].status == 0 else None, E["want"][q])
            seen.add(q)
        if len(tickets):
            pipe.release(tickets)
        assert time.time() - t0 < 60, "pipeline stalled: %d of %d" % (len(seen), N)
    assert seen == set(range(N)) and pipe.in_flight() == 0
    pipe.close()


def test_pipeline_rows_match_the_oracle_with_rows_reclaimed():
    through_the_pipeline(env(), footprint=False)


def test_footprint_rows_with_the_point_disc_match_the_oracle():
    through_the_pipeline(env(), footprint=True)


def test_batch_rows_match_the_oracle(monkeypatch):
    import pathplanning_amd as pa
    monkeypatch.setenv("PP_SEARCH_ROWS", "1")
    E = env()
    planner = pa.HybridAStarBatch(E["val"], max_batch=N, max_nodes=32768, search_rows=8)
    planner.initialize(E["table"])
    assert planner.search_rows == 8
    res = planner.search_batch(E["starts"], E["goals"], E["seeds"])
    assert len(res) == N
    for q in range(N):
        assert_is_the_oracles(q, res[q], planner.get_path_of(q)["poses"] if res[q].status == 0 else None, E["want"][q])
    planner.close()
