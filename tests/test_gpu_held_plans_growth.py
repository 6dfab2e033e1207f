"""-m gpu: the buffers of re-validation, stamp and locate GROW beside a query in flight (pp_pipeline_revalidate, pp_pipeline_stamp,
pp_pipeline_locate), as test_gpu_pipeline_postprocess.py checks for post-processing.  The construction is that test's: world
make_pair(256, 6, 3), the 40 queries of RandomState(42) with the one long search first, capacity 16, 8 search rows, device-array
submission.  Queries 1 .. 8 are held, then the long query 0 is submitted and not polled.  Every service is called with 2 tickets and then
with all 8 (every buffer of the service grows, and the outgrown ones must be parked, not freed: freeing waits for the grid), and once more
with all 8 when the long query has been drained (the parked buffers go).  The expected records are the batch form's on a HybridAStarBatch
that searched the same eight queries with the pipeline's non-holonomic table: the same kernel on the same plan records, so equality is
exact."""
import time

import numpy as np
import pytest

from gpu_common import make_pair, valid_random_poses
from test_gpu_pipeline_postprocess import drain

pytestmark = pytest.mark.gpu

SERVICES = ["revalidate", "stamp", "locate"]
HELD = 8
SPACING = 0.1


def fields(r):
    """a result record as a tuple of plain values, arrays as tuples"""
    return tuple(tuple(v) if hasattr(v, "__len__") else v for v in (getattr(r, name) for name, _ in r._fields_))


def same_records(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        for (name, _), x, y in zip(a._fields_, fields(a), fields(b)):
            assert x == y, "%s: record %d, field %s: %r != %r" % (what, k, name, x, y)


@pytest.fixture(scope="module")
def calls():
    """every call of the scenario, made once: {service: dict(two=, eight=, idle=, batch=, grow_s=, in_flight=)}"""
    import pathplanning_amd as pa
    import torch
    w, ms, val, ctx = make_pair(256, 6, 3)
    _, second, _, _ = make_pair(256, 6, 4, ctx=ctx)  # another obstacle set on the same grid: distance grid, int32 occupancy grid, validator tunables
    rng = np.random.RandomState(42)
    n = 40
    starts, goals = valid_random_poses(rng, w, n), valid_random_poses(rng, w, n)
    seeds = np.arange(n, dtype=np.uint64) + 900
    for a in (starts, goals, seeds):  # the one long search of this stream (4067 expansions in the oracle) is query 0
        a[[0, 10]] = a[[10, 0]]
    pipe = pa.HybridAStarPipeline(val, capacity=16, max_nodes=32768, search_rows=8)
    pipe.initialize()
    batch = pa.HybridAStarBatch(val, max_batch=HELD, max_nodes=32768)
    batch.initialize(pipe.nonholo_table())
    ref = batch.search_batch(starts[1:1 + HELD], goals[1:1 + HELD], seeds[1:1 + HELD])
    vehicles = starts[1:1 + HELD]  # every vehicle at its plan's start pose
    dev = torch.device("cuda", 0)
    d_starts, d_goals = torch.from_numpy(np.ascontiguousarray(starts)).to(dev), torch.from_numpy(np.ascontiguousarray(goals)).to(dev)
    d_seeds = torch.from_numpy(seeds.astype(np.int64)).to(dev)
    first, took = pipe.submit_dev(d_starts, d_goals, d_seeds, n=HELD, offset=1)
    assert took == HELD
    got = drain(pipe, HELD)
    held = [first + i for i in range(HELD)]  # in query order: ticket k is query 1 + k
    for k, t in enumerate(held):
        assert got[t].status == ref[k].status and got[t].n_expanded == ref[k].n_expanded
    long_one, took = pipe.submit_dev(d_starts, d_goals, d_seeds, n=1, offset=0)
    assert took == 1 and pipe.in_flight() == 1

    by_ticket = {
        "revalidate": lambda t: pipe.revalidate(t, map_set=second),
        "stamp": lambda t: pipe.stamp(t, map_set=second, values=2, spacing=SPACING),
        "locate": lambda t: pipe.locate(t, vehicles[:len(t)], spacing=SPACING),
    }
    out = {}
    for name in SERVICES:
        two = by_ticket[name](held[:2])
        t0 = time.time()
        eight = by_ticket[name](held)  # 8 plans after 2: every buffer of the service grows
        out[name] = dict(two=two, eight=eight, grow_s=time.time() - t0, in_flight=pipe.in_flight())
    drain(pipe, 1)
    assert pipe.in_flight() == 0
    for name in SERVICES:
        out[name]["idle"] = by_ticket[name](held)  # nothing in flight: the parked buffers are dropped
    out["revalidate"]["batch"] = batch.revalidate(map_set=second)
    out["stamp"]["batch"] = batch.stamp(map_set=second, values=2, spacing=SPACING)
    out["locate"]["batch"] = batch.locate(vehicles, spacing=SPACING)
    pipe.release(held + [long_one])
    assert pipe.free_slots() == 16
    pipe.close()
    batch.close()
    return out


@pytest.mark.parametrize("service", SERVICES)
def test_buffers_grow_beside_a_query_in_flight(calls, service):
    c = calls[service]
    print("a %s call that grows its buffers beside a query in flight: %.1f ms" % (service, 1e3 * c["grow_s"]))
    assert c["in_flight"] == 1  # (nothing was polled: the long query is still the grid's)
    assert len(c["two"]) == 2 and len(c["eight"]) == HELD
    assert any(r.status == 0 for r in c["eight"])
    same_records(c["eight"][:2], c["two"], service + ": the larger call against the smaller one")
    same_records(c["idle"], c["eight"], service + ": with nothing in flight against beside the long query")
    same_records(c["eight"], c["batch"], service + ": by ticket against the batch form")
    # a call that frees waits for the long search and then for the grid's idle waves (over a second while the host does not poll); one that
    # parks takes milliseconds: the bound of test_post_processing_beside_queries_in_flight_with_recycled_slots
    assert c["grow_s"] < 0.5
