"""CPU: the numpy restatement of a broad-phase call (tests/pair_restatement.py), which tests/test_gpu_pipeline_candidate_pairs.py compares the kernels
with, run alone on the ORACLE's plans of the shared 48-plan scene, over the cases of tests/test_delay_restatement_host.py with every pair
(pairs=None).  Checked without a GPU, at 1, 16, 64 and T lattice times per box:
 - the guarantee: tests/delay_restatement.py's delay call over the candidate list gives the records of the call over every pair, in every field;
 - every blocker pair of the call over every pair is listed;
 - the lists are selections: neither empty nor complete;
 - nesting: list(B = 1) is inside list(16) inside list(64) inside list(T), and list(D) inside list(D') for D <= D';
 - the levels of a delay call drop."""
import numpy as np

import conflict_restatement as CR
import delay_restatement as DR
import pair_restatement as PR
from test_conflict_restatement_host import LIM, profiles
from test_delay_restatement_host import cases
from test_locate_restatement_host import scene

FIELDS = ("status", "delay_steps", "n_tried", "blocker", "t_start", "t_block", "s_block")


def extended(traj):
    """the poses of delay_restatement's extended trajectories as the broad phase takes them: None for a plan without a trajectory"""
    return [t["poses"] if t["status"] >= 0 else None for t in traj]


def as_set(pairs):
    return {(int(a), int(b)) for a, b in pairs}


def test_over_the_candidate_list_a_delay_call_gives_the_records_of_the_call_over_every_pair():
    plans, rows = profiles()
    starts = scene()[1]
    dropped = 0
    for name, (which, _, t_start, discs, kw) in cases(starts).items():
        n = len(which)
        tau, traj, full = DR.deconflict([plans[q] for q in which], [rows[q] for q in which], t_start, None, discs, LIM["a_acc"], LIM["a_dec"], **kw)
        T, D = len(tau), kw["max_delay_steps"]
        s_of = [t.get("s") for t in traj]
        poses = extended(traj)
        blockers = {(r["blocker"], i) for i, r in enumerate(full) if r["blocker"] >= 0}
        before = None
        for B in sorted({1, 16, 64, T}):
            want = PR.candidate_pairs(poses, T, D, B, discs, kw["margin"])
            pairs = as_set(want["pairs"])
            assert 0 < len(pairs) < n * (n - 1) // 2, (name, B, len(pairs))
            assert blockers <= pairs, (name, B, blockers - pairs)
            assert before is None or before <= pairs, (name, B)  # (a longer block holds the shorter ones that make it up)
            before = pairs
            recs = DR.decide(traj, s_of, tau, T, D, n, [tuple(p) for p in want["pairs"]], discs, kw["margin"], t_start, kw["dt"])
            for i, (a, b) in enumerate(zip(recs, full)):
                assert all(a[k] == b[k] for k in FIELDS), (name, B, i, a, b)
            levels = (max(DR.levels(n, [tuple(p) for p in want["pairs"]])) + 1, max(DR.levels(n, None)) + 1)
            print("%s, B = %d: %d of %d pairs, %d boxes, %d of %d plans boxed, levels %d of %d" % (name, B, len(pairs), n * (n - 1) // 2, want["n_boxes"], want["n_boxed"], n,
                                                                                               levels[0], levels[1]))
            if B == 16:
                assert levels[0] <= levels[1]
                dropped += levels[0] < levels[1]
        # a larger largest delay widens every box: list(D') holds list(D) for D' <= D
        for smaller in sorted({0, D // 2} - {D}):
            k0 = CR.lattice(kw["t_from"], kw["t_to"], kw["dt"])[0]
            assert len(CR.times(k0 - smaller, T + smaller, kw["dt"])) == T + smaller
            narrow = PR.candidate_pairs([None if p is None else p[D - smaller:] for p in poses], T, smaller, 16, discs, kw["margin"])
            assert as_set(narrow["pairs"]) <= as_set(PR.candidate_pairs(poses, T, D, 16, discs, kw["margin"])["pairs"]), (name, smaller)
    assert dropped >= 8


def test_the_list_is_ascending_and_first_box_is_the_first_box_that_hits():
    plans, rows = profiles()
    starts = scene()[1]
    which, _, t_start, discs, kw = cases(starts)["nearest, hold-both"]
    tau, traj, _ = DR.deconflict([plans[q] for q in which], [rows[q] for q in which], t_start, [], discs, LIM["a_acc"], LIM["a_dec"], **kw)
    T, D = len(tau), kw["max_delay_steps"]
    want = PR.candidate_pairs(extended(traj), T, D, 16, discs, kw["margin"])
    pairs, first, box = want["pairs"], want["first_box"], want["boxes"]
    keys = pairs[:, 0].astype(np.int64) * len(which) + pairs[:, 1]
    assert (pairs[:, 0] < pairs[:, 1]).all() and (np.diff(keys) > 0).all()
    failed = [i for i, t in enumerate(traj) if t["status"] < 0]
    assert failed and not np.isin(pairs, failed).any() and np.isnan(box[failed]).all() and want["n_boxed"] <= len(which) - len(failed)
    for (i, j), b in zip(pairs, first):
        assert PR.can_meet(box[i, b], box[j, b], want["reach"]) and not any(PR.can_meet(box[i, k], box[j, k], want["reach"]) for k in range(b))
    assert len(set(first.tolist())) > 1
