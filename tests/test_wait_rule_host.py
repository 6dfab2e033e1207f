"""CPU: the rule of a call with waits at stops (pathplanning_amd/csrc/pp_wait_rule.hpp, the text k_wait_places and k_wait_level compile for the
device) run by tests/cpp/test_wait_rule.cpp -- a stand-alone program with its own main, built with g++ under the address and undefined-behaviour
sanitizers and run as a child process.  Nothing loaded into this interpreter runs under a sanitizer.

The program checks itself (see its head).  It also prints every value it computed, doubles as hexadecimal floats, and this file compares each with
tests/wait_restatement.py, the numpy restatement the GPU tests compare the kernels with, EXACTLY."""
import subprocess

import wait_restatement as WR


def run_program():
    from pathplanning_amd import build
    exe = build.build_wait_rule_test(verbose=False)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    return [ln.split() for ln in run.stdout.splitlines()]


LINES = None


def program(kind=None):
    global LINES
    if LINES is None:
        LINES = run_program()
    return LINES if kind is None else [ln[1:] for ln in LINES if ln[0] == kind]


def test_the_program_checks_itself_and_ends_clean():
    assert program()[-1] == ["wait", "rule", "ok"]


def test_the_position_under_a_wait_equals_the_restatement():
    lines = [[int(x) for x in ln] for ln in program("S")]
    seen = set()
    for T, D, a, d, c, at in lines:
        assert at == WR.source(c, a, d), (T, D, a, d, c)
        seen.add((T, D, a, d))
    for T, D in ((1, 0), (1, 3), (5, 3), (64, 65)):  # every c of every m, over a = 0, D, T + D - 1, T + D and d = 0, 1, D
        for a in {0, D, T + D - 1, T + D}:
            for d in {d for d in (0, 1, D) if d <= D}:
                assert (T, D, a, d) in seen and sorted({ln[4] for ln in lines if ln[:4] == [T, D, a, d]}) == list(range(D, T + D))
    assert any(at == -1 for *_, at in lines) and len(lines) == 4 * 3 * (1 + 1 + 5 + 64) - 4  # (d = 1 > D = 0 is left out)
    starts = [[int(x) for x in ln] for ln in program("W")]
    assert len(starts) >= 200 and all(at == c - d for D, d, c, at in starts)


def test_the_arrive_column_equals_the_restatement_at_and_one_ulp_either_side():
    lines = program("A")
    assert len(lines) == 5 * 8 * 3
    hit = 0
    for kE, columns, dt, t_start, t_arrive, a in lines:
        kE, columns, a = int(kE), int(columns), int(a)
        dt, t_start, t_arrive = float.fromhex(dt), float.fromhex(t_start), float.fromhex(t_arrive)
        assert a == WR.arrive_column(kE, columns, dt, t_start, t_arrive), (kE, columns, dt, t_start, t_arrive)
        hit += 0 < a < columns
    assert hit >= 30
    # a column's own time arrives at that column, one ulp more at the next one
    triples = [lines[i:i + 3] for i in range(0, len(lines), 3)]
    assert sum(int(lo[5]) == int(at[5]) and int(hi[5]) == int(at[5]) + 1 for lo, at, hi in triples) >= 8


def test_the_filters_equal_the_restatement():
    import numpy as np
    lines = [[int(x) for x in ln] for ln in program("F")]
    assert len(lines) == 30
    for row, N, a, D, columns, place, fixed in lines:
        every = np.zeros(1, dtype=WR.PLACE_DTYPE)
        every["row"], every["column"] = row, a
        assert place == len(WR.places_of(every, N, D, columns, 4)[0])
        if row >= 0:
            assert fixed == int(WR.places_of(every, N, D, columns, 4, fixed_row=row)[1] and row < N)
        else:
            assert fixed == 0
    assert sum(ln[5] for ln in lines) == 4 and sum(ln[6] for ln in lines) == 16


def test_the_candidate_order_equals_the_restatement():
    counts = {tuple(int(x) for x in ln[:3]): int(ln[3]) for ln in program("N")}
    assert len(counts) == 18
    for (D, S, P), n in counts.items():
        got = [(int(ln[4]), int(ln[5])) for ln in program("O") if (int(ln[0]), int(ln[1]), int(ln[2])) == (D, S, P)]
        assert [int(ln[3]) for ln in program("O") if (int(ln[0]), int(ln[1]), int(ln[2])) == (D, S, P)] == list(range(n))
        assert got == WR.candidates(D, bool(S), P) and len(got) == n


def test_the_shortcut_agrees_with_the_exhaustive_evaluation():
    lines = [[int(x) for x in ln] for ln in program("X")]
    assert len(lines) >= 2000
    for T, D, a, d, m0, skip, m in lines:
        assert skip == int(m0 >= 0 and a > m0 + D)
        if skip:
            assert m == m0
    assert sum(ln[5] for ln in lines) >= 100 and any(not ln[5] and ln[4] >= 0 and ln[6] != ln[4] for ln in lines)
