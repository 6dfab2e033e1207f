"""CPU: the rule of the space-time broad phase (pathplanning_amd/csrc/pp_pair_rule.hpp, the text k_plan_boxes and k_box_pairs compile for the device
and the host side of pp_pipeline_candidate_pairs runs) run by tests/cpp/test_pair_rule.cpp -- a stand-alone program with its own main, built with g++
under the address and undefined-behaviour sanitizers and run as a child process.  Nothing loaded into this interpreter runs under a sanitizer.

The program checks itself (see its head).  It also prints every value it computed -- doubles as their 64 bits -- and this file compares each with
tests/pair_restatement.py, the numpy restatement the GPU tests compare the kernels with, EXACTLY."""
import struct
import subprocess

import numpy as np

import footprint_ref as FR
import pair_restatement as PR


def run_program():
    from pathplanning_amd import build
    exe = build.build_pair_rule_test(verbose=False)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    return [ln.split() for ln in run.stdout.splitlines()]


LINES = None


def program():
    global LINES
    if LINES is None:
        LINES = run_program()
    return LINES


def dbl(word):
    return struct.unpack("<d", struct.pack("<Q", int(word, 16)))[0]


def word(value):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(value)))[0]


def test_the_program_checks_itself_and_ends_clean():
    assert program()[-1] == ["pair", "rule", "ok"]


def test_box_counts_and_column_ranges_equal_the_restatement():
    counts = [[int(x) for x in ln[1:]] for ln in program() if ln[0] == "N"]
    assert {(T, D) for T, _, D, _ in counts} == {(T, D) for T in (1, 63, 64, 65, 130) for D in (0, 1, 65)}
    for T in (1, 63, 64, 65, 130):
        assert {B for t, B, _, _ in counts if t == T} == {1, 16, 64, T, 1 << 20}
    for T, B, D, NB in counts:
        assert NB == PR.box_count(T, B)
    ranges = [[int(x) for x in ln[1:]] for ln in program() if ln[0] == "C"]
    assert len(ranges) == sum(NB for _, _, _, NB in counts)
    for T, B, D, b, first, last in ranges:
        assert (first, last) == PR.columns(b, B, T, D) and 0 <= first <= last < T + D
    assert [65, 64, 65, 1, 64, 129] in ranges and [130, 64, 0, 2, 128, 129] in ranges and [1, 1 << 20, 65, 0, 0, 65] in ranges


def test_the_reach_of_the_point_disc_and_of_car3_equals_the_restatement():
    discs = [[dbl(x) for x in ln[1:]] for ln in program() if ln[0] == "D"]
    assert len(discs) == 6
    for ox, oy, r, got in discs:
        assert word(got) == word(PR.disc_reach((ox, oy, r)))
    sets = {"point": [(0.0, 0.0, 1.0)], "CAR3": FR.CAR3, "skew": [(0.3, -0.4, 0.1), (-3.0, 4.0, 0.0)]}
    lines = [ln[1:] for ln in program() if ln[0] == "H"]
    assert {ln[0] for ln in lines} == set(sets) and len(lines) == 12
    for name, margin, R, reach in lines:
        assert word(max(PR.disc_reach(d) for d in sets[name])) == R and word(PR.reach(sets[name], dbl(margin))) == reach, (name, dbl(margin))
    assert word(PR.reach(FR.CAR3, 0.2)) in [ln[3] for ln in lines] and dbl(word(PR.reach(FR.CAR3, 0.2))) == (0.2 + 2 * (3.0 + float(np.float32(1.3)))) + 1e-6


def test_boxes_from_points_equal_the_restatement():
    sets, cur = [], None
    for ln in program():
        if ln[0] == "S":
            cur = dict(name=ln[1], n=int(ln[2]), points=[])
            sets.append(cur)
        elif ln[0] == "Q":
            cur["points"].append((dbl(ln[1]), dbl(ln[2])))
        elif ln[0] == "E":
            cur["box"] = ln[1:]
    assert [s["name"] for s in sets] == ["empty", "absent", "one", "gaps", "equal", "many"]
    for s in sets:
        assert len(s["points"]) == s["n"]
        poses = np.array([(x, y, 0.0) for x, y in s["points"]]).reshape(-1, 3)
        want = PR.boxes([poses], len(poses), 0, max(len(poses), 1))[0, 0] if len(poses) else np.full(4, np.nan)
        assert [word(v) for v in want] == s["box"], s["name"]
    by = {s["name"]: s for s in sets}
    assert all(np.isnan(dbl(w)) for w in by["empty"]["box"] + by["absent"]["box"]) and by["gaps"]["box"] == [word(v) for v in (-4.0, -1.0, 2.5, 9.0)]
    assert by["many"]["n"] == 200 and sum(np.isnan(x) for x, _ in by["many"]["points"]) == 20


def test_the_box_test_at_the_reach_one_ulp_below_and_one_ulp_above_equals_the_restatement():
    lines = [ln[1:] for ln in program() if ln[0] == "X"]
    assert len(lines) == 3 * (6 * 5 + 4)
    met = 0
    for ln in lines:
        a, b, reach, got = [dbl(x) for x in ln[0:4]], [dbl(x) for x in ln[4:8]], dbl(ln[8]), int(ln[9])
        assert got == int(PR.can_meet(a, b, reach)) == int(PR.can_meet(b, a, reach)), ln
        met += got
    assert 0 < met < len(lines)
    # exactly at, one ulp below and one ulp above the reach, with an empty box on either side
    reach = PR.reach([(0.0, 0.0, 1.0)], 0.5)
    a = [-1.0, -1.0, 0.0, 0.0]
    for g, want in ((reach, 1), (np.nextafter(reach, -np.inf), 1), (np.nextafter(reach, np.inf), 0)):
        for b in ([g, -0.5, g + 1.0, 0.5], [-0.5, g, 0.5, g + 1.0]):
            assert [word(v) for v in a + b] + [word(reach), str(want)] in lines
    nan = word(np.nan)
    assert [word(v) for v in a] + [nan] * 4 + [word(reach), "0"] in lines and [nan] * 4 + [word(v) for v in a] + [word(reach), "0"] in lines
