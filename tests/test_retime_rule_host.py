"""CPU: the arithmetic of a retime call (pathplanning_amd/csrc/pp_retime_rule.hpp, the text k_retime_tickets compiles for the device) run by
tests/cpp/test_retime_rule.cpp -- a stand-alone program with its own main, built with g++ without contraction under the address and
undefined-behaviour sanitizers and run as a child process.  Nothing loaded into this interpreter runs under a sanitizer.

The program checks itself (see its head): the order of the prefix, h(k) at a hold's row, before the first hold and behind the last, validity at
delta + w == 0 exactly and one ulp below, a hold at N - 1, monotone times inside one hold segment.  It also prints what it computed as hex floats, so
every double arrives bit for bit, and this file compares every printed value with tests/retime_restatement.py -- the numpy restatement the GPU tests
compare the kernel with -- EXACTLY."""
import subprocess

import numpy as np

import retime_restatement as RT

LINES = None


def program():
    global LINES
    if LINES is None:
        from pathplanning_amd import build
        exe = build.build_retime_rule_test(verbose=False)
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
        assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
        LINES = [ln.split() for ln in run.stdout.splitlines()]
    return LINES


def f(x):
    return np.float64(float.fromhex(x))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


PROFILES = None


def profiles():
    """[{name, n, a_acc, a_dec, rows, dwell: {r: delta}, cases: [{name, holds: [(row, seconds, status, P)], h: [..], t: [..]}]}]"""
    global PROFILES
    if PROFILES is None:
        PROFILES, cur, case = [], None, None
        for ln in program():
            if ln[0] == "Q":
                cur = dict(name=ln[1], n=int(ln[2]), a_acc=f(ln[3]), a_dec=f(ln[4]), rows=[], dwell={}, cases=[])
                PROFILES.append(cur)
            elif ln[0] == "R":
                cur["rows"].append([f(x) for x in ln[1:4]])
            elif ln[0] == "D":
                cur["dwell"][int(ln[1])] = f(ln[2])
            elif ln[0] == "C":
                case = dict(name=ln[1], count=int(ln[2]), holds=[], h=[], t=[])
                cur["cases"].append(case)
            elif ln[0] == "G":
                case["holds"].append((int(ln[1]), f(ln[2]), int(ln[3]), f(ln[4])))
            elif ln[0] == "K":
                case["h"].append(int(ln[2]))
            elif ln[0] == "T":
                case["t"].append(f(ln[2]))
        for q in PROFILES:
            q["rows"] = np.array(q["rows"])
    return PROFILES


def test_the_program_checks_itself_and_ends_clean():
    assert program()[-1] == ["retime", "rule", "ok"]
    by = {q["name"]: q for q in profiles()}
    assert by["short-40"]["n"] == 40 and by["long-200"]["n"] == 200 and by["two-standing"]["n"] == 2
    stops = np.flatnonzero(by["rows-63-64-65"]["rows"][:, 1] == 0.0).tolist()
    assert stops == [0, 63, 64, 65, 128, 149]
    for q in profiles():
        names = [c["name"] for c in q["cases"]]
        assert "none" in names and "last-row" in names and "every-stop" in names
        if q["n"] > 2:
            assert "moving-row" in names and any(n.startswith("minus-the-dwell-") for n in names) and any(n.startswith("one-ulp-below-") for n in names)
            assert any(n.startswith("offender-second-") for n in names)


def test_dwells_and_statuses_equal_the_restatement():
    checked = 0
    for q in profiles():
        for r, d in q["dwell"].items():
            assert bits(RT.dwell(q["rows"], r, q["a_acc"], q["a_dec"])) == bits(d), (q["name"], r)
        for c in q["cases"]:
            for row, w, status, _ in c["holds"]:
                assert RT.hold_status(q["rows"], row, w, q["a_acc"], q["a_dec"]) == status, (q["name"], c["name"], row)
                checked += 1
            if c["name"].startswith("minus-the-dwell-"):
                (row, w, status, _), = c["holds"]
                assert status == 0 and q["dwell"][row] + w == 0.0 and q["dwell"][row] > 0.1
            if c["name"].startswith("one-ulp-below-"):
                (row, w, status, _), = c["holds"]
                assert status == -3 and w == np.nextafter(-q["dwell"][row], -np.inf)
            if c["name"].startswith("moving-row"):
                assert [h[2] for h in c["holds"]] == [-2]
    assert checked > 100


def test_prefix_hold_of_and_rewritten_times_equal_the_restatement_bit_for_bit():
    rewritten = 0
    for q in profiles():
        for c in q["cases"]:
            here = (q["name"], c["name"])
            holds = [(row, w) for row, w, _, _ in c["holds"]]
            assert len(holds) == c["count"]
            assert np.array_equal(bits(RT.prefix([w for _, w in holds])), bits([h[3] for h in c["holds"]])), here
            at = np.array([row for row, _ in holds], dtype=np.int64)
            assert np.array_equal(np.searchsorted(at, np.arange(q["n"]), side="right") - 1, c["h"]), here
            rec, after = RT.retime(q["rows"], holds, q["a_acc"], q["a_dec"], first=5)
            first_bad = next((k for k, h in enumerate(c["holds"]) if h[2] != 0), None)
            if first_bad is not None:
                assert c["t"] == [] and rec["status"] == c["holds"][first_bad][2] and rec["bad_hold"] == 5 + first_bad and rec["first_row"] == -1, here
                assert after.tobytes() == q["rows"].tobytes() and rec["held"] == 0.0 and rec["duration"] == rec["duration_before"] == q["rows"][-1, 2], here
                continue
            assert np.array_equal(bits(after[:, 2]), bits(c["t"])), here
            assert after[:, :2].tobytes() == q["rows"][:, :2].tobytes(), here
            assert rec["status"] == 0 and rec["bad_hold"] == -1 and rec["n_holds"] == len(holds) and rec["first_row"] == (holds[0][0] if holds else -1), here
            assert rec["duration_before"] == q["rows"][-1, 2] and rec["duration"] == after[-1, 2], here
            if holds:
                assert bits(rec["held"]) == bits(c["holds"][-1][3]), here
                lo = holds[0][0]
                assert after[:lo].tobytes() == q["rows"][:lo].tobytes(), here
                for a, b in zip(list(at), list(at[1:]) + [q["n"]]):  # inside one hold segment the times never decrease
                    assert (np.diff(after[a:b, 2]) >= 0.0).all(), here
            if c["name"] == "last-row":
                assert after[:-1].tobytes() == q["rows"][:-1].tobytes() and after[-1, 2] == q["rows"][-1, 2] + 2.5, here
            rewritten += len(c["t"])
    assert rewritten > 2000


def test_a_call_of_several_plans_numbers_the_offender_in_the_calls_list():
    by = {q["name"]: q for q in profiles()}
    a, b = by["junction-cusp-dwell"], by["short-40"]
    holds = np.array([(0, 6, 0.75), (0, 9, 0.25), (2, 7, 1.0), (2, 8, 1.0), (2, 14, 1.0)], dtype=RT.HOLD_DTYPE)  # (row 8 of short-40 moves)
    recs, after = RT.retime_call([a["rows"], None, b["rows"], b["rows"]], holds, 1.5, 2.5)
    assert recs["status"].tolist() == [0, -1, -2, 0] and recs["bad_hold"].tolist() == [-1, -1, 3, -1] and recs["n_holds"].tolist() == [2, 0, 3, 0]
    assert after[1] is None and after[2].tobytes() == b["rows"].tobytes() and after[3].tobytes() == b["rows"].tobytes()
    assert recs[0]["held"] == 1.0 and recs[0]["first_row"] == 6 and np.array_equal(after[0][:, 2] - a["rows"][:, 2] > 0.7, np.arange(10) >= 6)
    assert recs[1].tobytes() == np.array((-1, 0, 0, -1, 0.0, 0.0, 0.0), dtype=RT.RESULT_DTYPE).tobytes()
