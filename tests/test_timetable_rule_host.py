"""CPU: the arithmetic of a timetable call (pathplanning_amd/csrc/pp_timetable_rule.hpp, the text k_timetable_tickets compiles for the device) run by
tests/cpp/test_timetable_rule.cpp -- a stand-alone program with its own main, built with g++ without contraction under the address and
undefined-behaviour sanitizers and run as a child process.  Nothing loaded into this interpreter runs under a sanitizer.

The program checks itself (see its head).  It also prints what it computed as hex floats, so every double arrives bit for bit, and this file compares
every printed value with tests/timetable_restatement.py -- the numpy restatement the GPU tests compare the kernel with -- EXACTLY."""
import subprocess

import numpy as np

import timetable_restatement as TT

HAND_MADE = ("rest-to-rest", "junction-cusp-dwell", "two-standing", "standing-dwell-standing", "one", "one-at-zero", "all-at-one-place", "random-11")
ADDED = ("starts-moving", "window-from-7.5", "plateau")


def run_program():
    from pathplanning_amd import build
    exe = build.build_timetable_rule_test(verbose=False)
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
    return np.float64(float.fromhex(x) if x not in ("inf", "-inf", "nan", "-nan") else float(x))


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


PROFILES = None


def profiles():
    global PROFILES
    if PROFILES is None:
        PROFILES, cur = [], None
        for ln in program():
            if ln[0] == "Q":
                cur = dict(name=ln[1], n=int(ln[2]), a_acc=f(ln[3]), a_dec=f(ln[4]), rows=[], stops=[], T=[], S=[], N=[], worst=None)
                PROFILES.append(cur)
            elif ln[0] == "R":
                cur["rows"].append([f(x) for x in ln[1:4]])
            elif ln[0] == "P":
                cur["stops"].append((int(ln[1]), int(ln[2]), f(ln[3]), f(ln[4]), f(ln[5])))
            elif ln[0] in "TS":
                cur[ln[0]].append((f(ln[1]), int(ln[2]), int(ln[3])) + tuple(f(x) for x in ln[4:8]))
            elif ln[0] == "N":
                cur["N"].append(tuple(int(x) for x in ln[1:4]))
            elif ln[0] == "W":
                cur["worst"] = f(ln[2])
        for q in PROFILES:
            q["rows"] = np.array(q["rows"])
    return PROFILES


def test_the_program_checks_itself_and_ends_clean():
    assert program()[-1] == ["timetable", "rule", "ok"]
    names = [q["name"] for q in profiles()]
    for need in HAND_MADE + ADDED:
        assert need in names, need
    worst = max(q["worst"] for q in profiles())
    print("worst |s(t(s)) - s| over %d profiles: %.3g m" % (len(names), worst))
    assert worst <= 1e-9


def test_the_profiles_are_the_ones_asked_for():
    by = {q["name"]: q for q in profiles()}
    cusp = by["junction-cusp-dwell"]["rows"]
    assert (np.diff(cusp[:, 0]) == 0.0).sum() == 2 and abs((cusp[6, 2] - cusp[5, 2]) - 1.25) < 1e-12  # a junction, and a cusp stop that dwells 1.25 s
    assert by["starts-moving"]["rows"][0, 1] > 0.0 and by["window-from-7.5"]["rows"][0, 0] == 7.5
    plateau = by["plateau"]["rows"]
    assert list(np.flatnonzero(plateau[:, 1] == 0.0)) == [0, 2, 3, 4, 6]  # three standing samples in a row
    assert len(by["one"]["rows"]) == 1 and by["two-standing"]["rows"][1, 2] > 2.0
    # the look-ups the issue lists: every s_j and t_j and their neighbours in double, before and behind, inside a dwell, either side of the triangle's x
    for q in profiles():
        rows, asked_t, asked_s = q["rows"], np.array([x[0] for x in q["T"]]), np.array([x[0] for x in q["S"]])
        for col, asked in ((2, asked_t), (0, asked_s)):
            have = set(bits(asked).tolist())
            for x in rows[:, col]:
                assert {int(bits(x)), int(bits(np.nextafter(x, -np.inf))), int(bits(np.nextafter(x, np.inf)))} <= have, (q["name"], col, x)
            assert (asked < rows[0, col]).any() and (asked > rows[-1, col]).any()
    dwell = [(u, st, j, s, t, v, a) for u, st, j, s, t, v, a in by["junction-cusp-dwell"]["T"] if cusp[5, 2] < u < cusp[6, 2]]
    assert len(dwell) > 50 and all(s == 2.0 and v == 0.0 and a == 0.0 for _, _, _, s, _, v, a in dwell)
    two = by["two-standing"]
    x = 2.0 * two["a_dec"] / (two["a_acc"] + two["a_dec"])
    sides = {float(a) for s, st, j, s2, t, v, a in two["S"] if 0.0 < s < 2.0 and abs(s - x) < 1e-12}
    assert sides == {float(two["a_acc"]), -float(two["a_dec"])}


def test_stops_equal_the_restatement_bit_for_bit():
    total = 0
    for q in profiles():
        mine = TT.stops(q["rows"], q["a_acc"], q["a_dec"])
        got = q["stops"]
        assert len(mine) == len(got), q["name"]
        assert [g[0] for g in got] == list(range(len(got))) and [g[1] for g in got] == mine["row"].tolist(), q["name"]
        for k, name in ((2, "s"), (3, "t_arrive"), (4, "t_depart")):
            assert np.array_equal(bits([g[k] for g in got]), bits(mine[name])), (q["name"], name)
        assert (mine["t_arrive"] <= mine["t_depart"]).all()
        total += len(got)
    assert total > 100
    by = {q["name"]: q for q in profiles()}
    st = TT.stops(by["junction-cusp-dwell"]["rows"], 1.5, 2.5)
    assert st["row"].tolist() == [5, 6] and abs((st["t_depart"][1] - st["t_arrive"][1]) - 1.25) < 1e-12 and st["t_arrive"][0] == st["t_depart"][0]
    assert TT.stops(by["one"]["rows"], 1.5, 2.5)["row"].tolist() == [0] and len(TT.stops(by["one-at-zero"]["rows"], 1.5, 2.5)) == 0


def test_look_ups_equal_the_restatement_bit_for_bit():
    asked = 0
    for q in profiles():
        for key, fn in (("T", TT.by_time), ("S", TT.by_length)):
            got = q[key]
            value = np.array([g[0] for g in got])
            status, row, s, t, v, a = fn(q["rows"], value, q["a_acc"], q["a_dec"])
            assert np.array_equal(status, [g[1] for g in got]), (q["name"], key)
            bad = np.flatnonzero(row != np.array([g[2] for g in got]))
            assert len(bad) == 0, (q["name"], key, got[bad[0]], row[bad[0]])
            for k, mine, name in ((3, s, "s"), (4, t, "t"), (5, v, "v"), (6, a, "a")):
                bad = np.flatnonzero(bits(mine) != bits([g[k] for g in got]))
                assert len(bad) == 0, (q["name"], key, name, got[bad[0]], mine[bad[0]])
            asked += len(got)
    assert asked > 40000


def test_next_stop_equals_the_restatement():
    asked = 0
    for q in profiles():
        every = TT.stops(q["rows"], q["a_acc"], q["a_dec"])
        inside = [(listed, j, nxt) for listed, j, nxt in q["N"] if 0 <= j < q["n"]]
        for listed in sorted({x[0] for x in inside}):
            j = np.array([x[1] for x in inside if x[0] == listed])
            # (a look-up of the whole call whose row is j: the by-length look-up at s_j lands on the last row of equal arc lengths, so ask the search itself)
            k = np.searchsorted(every["row"][:listed], j, side="right")
            want = np.where(k < listed, k, -1)
            assert np.array_equal(want, [x[2] for x in inside if x[0] == listed]), (q["name"], listed)
            asked += len(j)
    assert asked > 1000
    # ... and through the whole restated call: the plan record, the list cut at max_stops, the distances to the next stop
    q = {p["name"]: p for p in profiles()}["plateau"]
    rec, listed, out, _ = TT.timetable(False, q["rows"], q["rows"][:, 0], "length", q["a_acc"], q["a_dec"], max_stops=3)
    assert (rec["status"], rec["n_samples"], rec["n_stops"], rec["n_listed"]) == (0, 7, 5, 3) and listed["row"].tolist() == [0, 2, 3]
    assert out["row"].tolist() == [0, 1, 2, 3, 4, 5, 6] and out["next_stop"].tolist() == [1, 1, 2, -1, -1, -1, -1]
    assert out["s_to_stop"][0] == 1.0 and out["t_to_stop"][1] == listed["t_arrive"][1] - out["t"][1] and out["t_remaining"][6] == 0.0
    rec, listed, out, _ = TT.timetable(None, None, [0.0, 1.0], "time", 1.5, 2.5)
    assert rec["status"] == -1 and out["status"].tolist() == [-1, -1] and not out["s"].any() and len(listed) == 0
