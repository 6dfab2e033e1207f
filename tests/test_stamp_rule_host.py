"""CPU: the stamp's sample schedule and cell rule (pathplanning_amd/csrc/pp_stamp_rule.hpp, the text k_stamp_tickets compiles for the device)
run by tests/cpp/test_stamp_rule.cpp -- a stand-alone program built with g++ under the address and undefined-behaviour sanitizers and run as a
child process -- against a restatement in numpy written here from the definition in include/pp_hip.h.  The program prints its inputs and
outputs as hex floats, so every double arrives bit for bit, and everything is integer and double arithmetic without libm: equality is exact.

Checked: the step count n = L > 0 ? ceil(L / spacing) : 0 and the ratios k / n (L == 0, L < spacing, L an exact multiple of spacing, one
step beyond a multiple, random pairs, a NaN and a negative length, the cap); the clipped row and column range of a disc against grids with
non-zero origins (inside, partly and wholly outside, R below half a cell, infinite and NaN centres, the whole grid) -- it is the formula's,
and no cell outside it passes the centre test; the centre test of every cell inside it."""
import math
import subprocess

import numpy as np

MAX_STEPS = 1 << 19


def run_program():
    from pathplanning_amd import build
    exe = build.build_stamp_rule_test(verbose=False)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    return [ln.split() for ln in run.stdout.splitlines()]


LINES = None


def lines(kind):
    global LINES
    if LINES is None:
        LINES = run_program()
    return [ln[1:] for ln in LINES if ln[0] == kind]


def f(x):
    return float.fromhex(x) if x not in ("nan", "-nan", "inf", "-inf") else float(x.lstrip("-") if "nan" in x else x)


def steps(L, spacing):
    if not L > 0.0:
        return 0
    q = L / spacing
    return MAX_STEPS if not q < MAX_STEPS else int(math.ceil(q))


def test_sample_counts_and_ratios():
    cases = lines("S")
    assert len(cases) >= 150
    seen = set()
    for c in cases:
        L, spacing, n = f(c[0]), f(c[1]), int(c[2])
        assert n == steps(L, spacing), (L, spacing, n)
        ratios = np.array([f(x) for x in c[3:]])
        shown = min(n, 4096)
        assert len(ratios) == shown + 1
        want = np.arange(shown + 1, dtype=np.float64) / np.float64(n) if n else np.zeros(1)
        assert np.array_equal(ratios, want), (L, spacing)
        assert ratios[0] == 0.0 and (n == 0 or shown < n or ratios[-1] == 1.0)
        if n and n < MAX_STEPS:
            assert (n - 1) * spacing < L <= n * spacing or math.isclose(L, n * spacing, rel_tol=1e-15) or math.isclose(L, (n - 1) * spacing, rel_tol=1e-15)
        seen.add("zero" if L == 0 else "none" if not L > 0 else "below" if L < spacing else "multiple" if (L / spacing) == int(L / spacing) else "fraction")
        if n == MAX_STEPS:
            seen.add("capped")
    assert seen == {"zero", "none", "below", "multiple", "fraction", "capped"}, seen


def axis_range(c, R, origin, res, n):
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.float64(((np.float64(c) - R) - origin) / res - 1.0)
        b = np.float64(((np.float64(c) + R) - origin) / res + 1.0)
    if np.isnan(a) or np.isnan(b):
        return 0, -1
    lo = (int(a) if a < n else n) if a > 0.0 else 0
    hi = (int(b) if b >= 0.0 else -1) if b < n else n - 1
    return lo, hi


def test_clipped_ranges_and_the_centre_test():
    cases = lines("C")
    assert len(cases) >= 250
    kinds = set()
    for c in cases:
        rows, cols = int(c[0]), int(c[1])
        res, gx, gy, cx, cy, R = (f(x) for x in c[2:8])
        r0, r1, c0, c1 = (int(x) for x in c[8:12])
        assert (r0, r1) == axis_range(cx, R, gx, res, rows) and (c0, c1) == axis_range(cy, R, gy, res, cols), c[:12]
        assert 0 <= r0 and r1 <= rows - 1 and 0 <= c0 and c1 <= cols - 1
        # the centre test of every cell of the grid, in the order the definition writes it
        with np.errstate(invalid="ignore", over="ignore"):
            dx = (gx + (np.arange(rows, dtype=np.float64) + 0.5) * res) - cx
            dy = (gy + (np.arange(cols, dtype=np.float64) + 0.5) * res) - cy
            covered = dx[:, None] * dx[:, None] + dy[None, :] * dy[None, :] <= R * R
        inside = np.zeros_like(covered)
        if r0 <= r1 and c0 <= c1:
            inside[r0:r1 + 1, c0:c1 + 1] = True
            got = np.array([ch == "1" for ch in c[12]]).reshape(r1 - r0 + 1, c1 - c0 + 1)
            assert np.array_equal(got, covered[r0:r1 + 1, c0:c1 + 1]), c[:12]
        else:
            assert c[12] == "-"
        assert not (covered & ~inside).any(), ("a covered cell outside the range", c[:12])
        n = int(covered.sum())
        whole = math.isfinite(cx) and math.isfinite(cy) and gx + R <= cx <= gx + rows * res - R and gy + R <= cy <= gy + cols * res - R
        kinds.add("empty range" if not inside.any() else "none covered" if n == 0 else "inside" if whole else "clipped")
        if R < 0.5 * res:
            kinds.add("small " + ("hit" if n else "miss"))
            assert n <= 1
        if n == rows * cols:
            kinds.add("whole grid")
    assert kinds == {"empty range", "none covered", "inside", "clipped", "small hit", "small miss", "whole grid"}, kinds


def test_the_small_pieces():
    assert lines("W") == [["1", "0", "1", "0"]]
    (r, s), = lines("R")
    assert f(r) == float(np.float32(1.0)) + float(np.float32(0.12)) and f(s) == 3.0 + 0.5 * 0.7
