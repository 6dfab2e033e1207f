"""A broad-phase call (include/pp_hip.h, "the pairs that can meet") restated in numpy, for tests/test_gpu_pipeline_candidate_pairs.py,
tests/test_pair_restatement_host.py and tests/test_pair_rule_host.py.  It shares nothing with the kernels or with pp_pair_rule.hpp: the boxes are
nanmin / nanmax over slices of the extended trajectory's poses (a [T + D, 3] array per plan, NaN where the plan is absent), the reach and the rule
are written here from the header, and the list is a plain double loop in ascending (i, j).

Nothing here is ever undecided: a box is a min and a max of given doubles, the test is one subtraction and one comparison per axis and direction."""
import numpy as np

MAX_TIMES_PER_BOX = 1 << 20
MAX_BOXES = 1 << 26


def box_count(T, B):
    return -(-int(T) // int(B))


def columns(b, B, T, D):
    """(first, last) column of the extended trajectory that box b covers: the lattice times b B .. min(b B + B, T) - 1 under every delay 0 .. D"""
    return b * B, min(b * B + B, T) - 1 + D


def disc_reach(disc):
    ox, oy, r = np.float64(disc[0]), np.float64(disc[1]), np.float64(np.float32(disc[2]))
    return np.sqrt(ox * ox + oy * oy) + r


def reach(discs, margin):
    """(margin + (R + R)) + 1e-6, R the largest disc_reach"""
    R = max(disc_reach(d) for d in discs)
    return float((np.float64(margin) + (R + R)) + np.float64(1e-6))


def boxes(poses, T, D, B):
    """[n, NB, 4]: (xmin, ymin, xmax, ymax) per plan and box, NaN where the plan is present at none of the box's columns; poses[i] is [T + D, 3] or None
    (no trajectory: status -1)"""
    NB = box_count(T, B)
    out = np.full((len(poses), NB, 4), np.nan)
    for i, p in enumerate(poses):
        if p is None:
            continue
        p = np.asarray(p, dtype=np.float64)
        assert p.shape[0] == T + D
        for b in range(NB):
            c0, c1 = columns(b, B, T, D)
            xy = p[c0:c1 + 1, :2]
            xy = xy[~np.isnan(xy[:, 0])]
            if len(xy):
                out[i, b] = (xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max())
    return out


def can_meet(a, b, reach_):
    """the two-axis test of two boxes (xmin, ymin, xmax, ymax)"""
    if np.isnan(a[0]) or np.isnan(b[0]):
        return False
    gx = max(a[0] - b[2], b[0] - a[2])
    gy = max(a[1] - b[3], b[1] - a[3])
    return not gx > reach_ and not gy > reach_


def listed(box, reach_):
    """(pairs [P, 2] int32 ascending in (i, j), first_box [P] int32) of the boxes [n, NB, 4]"""
    n, NB = box.shape[:2]
    pairs, first = [], []
    reach_ = np.float64(reach_)
    for i in range(n):
        if n - i - 1 == 0:
            continue
        there = ~np.isnan(box[i, :, 0])[None, :] & ~np.isnan(box[i + 1:, :, 0])  # [n - i - 1, NB]
        with np.errstate(invalid="ignore"):
            gx = np.maximum(box[i, :, 0][None] - box[i + 1:, :, 2], box[i + 1:, :, 0] - box[i, :, 2][None])
            gy = np.maximum(box[i, :, 1][None] - box[i + 1:, :, 3], box[i + 1:, :, 1] - box[i, :, 3][None])
            hit = there & ~(gx > reach_) & ~(gy > reach_)
        for k in np.flatnonzero(hit.any(axis=1)):
            pairs.append((i, i + 1 + int(k)))
            first.append(int(np.argmax(hit[k])))
    return np.array(pairs, dtype=np.int32).reshape(-1, 2), np.array(first, dtype=np.int32)


def candidate_pairs(poses, T, D, B, discs, margin):
    """what a call owes: pairs, first_box, boxes, n_found, n_boxes, n_boxed and reach"""
    assert 1 <= B <= MAX_TIMES_PER_BOX and len(poses) * box_count(T, B) <= MAX_BOXES
    box = boxes(poses, T, D, B)
    r = reach(discs, margin)
    pairs, first = listed(box, r)
    return dict(pairs=pairs, first_box=first, boxes=box, n_found=len(pairs), n_boxes=box.shape[1], n_boxed=int((~np.isnan(box[:, :, 0])).any(axis=1).sum()), reach=r)
