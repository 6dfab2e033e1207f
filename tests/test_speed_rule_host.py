"""CPU: the arithmetic of a speed profile (pathplanning_amd/csrc/pp_speed_rule.hpp, the text k_speed_profile_tickets compiles for the device) run by
tests/cpp/test_speed_rule.cpp -- a stand-alone program with its own main, built with g++ without contraction under the address and undefined-behaviour
sanitizers and run as a child process.  Nothing loaded into this interpreter runs under a sanitizer.

The program checks itself: the closed form of the two one-sided envelopes against a plain sequential forward-then-backward sweep (hand-made sequences
to 1e-12 relative; random ones to that plus the rounding of the keys, derived in the program), the step between two standing samples, ds == 0, N == 1
with v_start and v_end, denormal and huge arc lengths.  It also prints what it computed as hex floats, so every double arrives bit for bit, and this
file compares that with tests/speed_restatement.py -- the numpy restatement the GPU tests compare the kernel with -- EXACTLY: w, e, v and (both sides
sum in sample order) t."""
import subprocess

import numpy as np

import speed_restatement as V


def run_program():
    from pathplanning_amd import build
    exe = build.build_speed_rule_test(verbose=False)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    return [ln.split() for ln in run.stdout.splitlines()]


LINES = None


def program():
    global LINES
    if LINES is None:
        LINES = run_program()
    return LINES


def f(x):
    return np.float64(float.fromhex(x) if x not in ("inf", "-inf") else float(x))


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def sequences():
    out, cur = [], None
    for ln in program():
        if ln[0] == "Q":
            cur = dict(name=ln[1], n=int(ln[2]), a_acc=f(ln[3]), a_dec=f(ln[4]), v_start=f(ln[5]), v_end=f(ln[6]), dwell=f(ln[7]), rows=[])
            out.append(cur)
        elif ln[0] == "P":
            cur["rows"].append([f(ln[1]), f(ln[2]), float(ln[3])] + [f(x) for x in ln[4:8]])
    return out


def test_the_program_checks_itself_and_ends_clean():
    assert program()[-1] == ["speed", "rule", "ok"]


def test_the_sequences_equal_the_restatement_bit_for_bit():
    seqs = sequences()
    names = [q["name"] for q in seqs]
    for need in ("rest-to-rest", "bend-cusp-reverse", "one-a", "one-b", "one-c", "two-standing", "denormal", "denormal-moving", "huge", "huge-1e300", "random-39"):
        assert need in names, need
    samples = 0
    for q in seqs:
        rows = np.array(q["rows"])
        assert len(rows) == q["n"]
        s, cap, cusp = rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2] != 0
        lim = V.limits(a_acc=float(q["a_acc"]), a_dec=float(q["a_dec"]), dwell=float(q["dwell"]))
        w, e, v, t = V.envelope_and_times(s, cap, cusp, lim, float(q["v_start"]), float(q["v_end"]))
        for name, mine, theirs in (("w", w, rows[:, 3]), ("e", e, rows[:, 4]), ("v", v, rows[:, 5]), ("t", t, rows[:, 6])):
            assert np.array_equal(bits(mine), bits(theirs)), (q["name"], name, int(np.flatnonzero(bits(mine) != bits(theirs))[0]))
        samples += len(rows)
    assert samples > 5000
    # what the hand-made ones are for
    by = {q["name"]: np.array(q["rows"]) for q in seqs}
    rest = by["rest-to-rest"]
    assert rest[0, 5] == 0.0 and rest[-1, 5] == 0.0 and rest[:, 5].max() == 5.0  # from rest to the cap and back to rest
    assert abs(rest[1, 4] - 2.0 * 1.5 * 0.1) < 1e-12 and abs(rest[-2, 4] - 2.0 * 2.5 * 0.1) < 1e-12  # a_acc at the front, a_dec at the back
    bend = by["bend-cusp-reverse"]
    assert (np.diff(bend[:, 0]) == 0.0).sum() == 11 and bend[:, 2].sum() == 1  # every junction twice; one cusp stop
    k = int(np.flatnonzero(bend[:, 2])[0])
    assert bend[k, 5] == 0.0 and bend[k - 1, 5] == 0.0 and abs((bend[k, 6] - bend[k - 1, 6]) - 1.25) < 1e-12  # standing on both sides of ds == 0: the dwell alone
    assert bend[0, 5] == 1.0 and bend[-1, 5] == 0.5  # v_start and v_end
    assert (by["one-a"][0, 5], by["one-b"][0, 5], by["one-c"][0, 5]) == (1.0, 1.0, 0.5)
    two = by["two-standing"]
    assert two[0, 5] == 0.0 and two[1, 5] == 0.0 and two[1, 6] > 2.0  # 2 m from rest to rest takes more than 2 s at these limits


def test_the_step_times_equal_the_definition():
    steps = [[f(x) for x in ln[1:]] for ln in program() if ln[0] == "T"]
    assert len(steps) >= 49
    kinds = set()
    for ds, v0, v1, a, d, got in steps:
        if ds == 0.0:
            want, kind = np.float64(0.0), "ds == 0"
        elif v0 + v1 > 0.0:
            want, kind = (np.float64(2.0) * ds) / (v0 + v1), "moving"
        else:
            x = ds * d / (a + d)
            want, kind = np.sqrt(np.float64(2.0) * x / a) + np.sqrt(np.float64(2.0) * (ds - x) / d), "standing"
        assert bits(want) == bits(got), (ds, v0, v1, got, want)
        kinds.add(kind)
    assert kinds == {"ds == 0", "moving", "standing"}


def test_directions_cusps_and_caps_equal_the_definition():
    lines = program()
    carried = {(int(a), int(b)): int(c) for k, a, b, c in (ln for ln in lines if ln[0] == "D")}
    cusp = {(int(a), int(b)): int(c) for k, a, b, c in (ln for ln in lines if ln[0] == "U")}
    assert len(carried) == 9 and len(cusp) == 9
    for own in (-1, 0, 1):
        for previous in (-1, 0, 1):
            assert carried[(own, previous)] == (previous if own == 0 else own)
            assert cusp[(own, previous)] == int(own != 0 and previous != 0 and own != previous)
    caps = [ln[1:] for ln in lines if ln[0] == "K"]
    assert len(caps) == 60
    seen = set()
    for direction, kappa, cl, gain, floor, got in caps:
        direction, kappa, cl, gain, floor, got = int(direction), f(kappa), np.float32(f(cl)), f(gain), f(floor), f(got)
        c = np.float64(5.0 if direction == 1 else 2.0)
        if kappa > 0.0:
            c = min(c, np.sqrt(np.float64(2.0) / kappa))
        if gain > 0.0:
            c = min(c, floor + gain * np.float64(cl))
        assert bits(c) == bits(got), (direction, kappa, cl, gain, floor, got, c)
        seen.add((direction, bool(kappa > 0.0), bool(gain > 0.0)))
    assert len(seen) >= 8
