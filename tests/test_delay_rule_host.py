"""CPU: the rule of a delay call (pathplanning_amd/csrc/pp_delay_rule.hpp, the text k_delay_level compiles for the device and the host side of
pp_pipeline_deconflict runs) run by tests/cpp/test_delay_rule.cpp -- a stand-alone program with its own main, built with g++ under the address and
undefined-behaviour sanitizers and run as a child process.  Nothing loaded into this interpreter runs under a sanitizer.

The program checks itself (see its head).  It also prints every value it computed -- all of them integers -- and this file compares each with
tests/delay_restatement.py, the numpy restatement the GPU tests compare the kernel with, EXACTLY."""
import subprocess

import delay_restatement as DR


def run_program():
    from pathplanning_amd import build
    exe = build.build_delay_rule_test(verbose=False)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    return [ln.split() for ln in run.stdout.splitlines()]


LINES = None


def program():
    global LINES
    if LINES is None:
        LINES = run_program()
    return LINES


def graphs():
    out, cur = [], None
    for ln in program():
        if ln[0] == "G":
            cur = dict(name=ln[1], n=int(ln[2]), n_pairs=int(ln[3]), listed=ln[4] == "1", pairs=[])
            out.append(cur)
        elif ln[0] == "P":
            cur["pairs"].append((int(ln[1]), int(ln[2])))
        elif ln[0] in "ONVFM" and len(ln[0]) == 1:
            cur[ln[0]] = [int(x) for x in ln[1:]]
    return out


def test_the_program_checks_itself_and_ends_clean():
    assert program()[-1] == ["delay", "rule", "ok"]


def test_the_column_mapping_equals_the_restatement():
    lines = [[int(x) for x in ln[1:]] for ln in program() if ln[0] == "C"]
    assert len(lines) >= 500
    seen = set()
    for T, D, d, m, c in lines:
        assert c == DR.column(m, D, d) and 0 <= c < T + D
        seen.add(("d=0" if d == 0 else "") + ("d=D" if d == D else "") + ("D=0" if D == 0 else "") + ("T=1" if T == 1 else ""))
    assert {"d=0", "d=D", "d=0d=DD=0", "d=0T=1", "d=DT=1", "d=0d=DD=0T=1"} <= seen, seen
    assert [1, 0, 0, 0, 0] in lines and [1, (1 << 20) - 1, 0, 0, (1 << 20) - 1] in lines and [1 << 20, 0, 0, (1 << 20) - 1, (1 << 20) - 1] in lines


def test_keys_and_their_order_equal_the_restatement():
    keys = [[int(x) for x in ln[1:]] for ln in program() if ln[0] == "K"]
    assert len(keys) >= 60
    for m, n, j, k, m_back, j_back in keys:
        assert k == DR.key(m, n, j) < 2 ** 64 - 1 and (m_back, j_back) == (m, j) == divmod(k, n)
    orders = [[int(x) for x in ln[1:]] for ln in program() if ln[0] == "B"]
    assert len(orders) == 37
    assert all(b == int(ka < kb) for ka, kb, b in orders)
    assert sum(ka == kb for ka, kb, _ in orders) >= 7 and not any(b for ka, kb, b in orders if ka == kb)  # ties: neither is before the other


def test_partner_lists_levels_and_members_equal_the_restatement():
    from pathplanning_amd.planner import delay_levels
    by = {g["name"]: g for g in graphs()}
    assert set(by) == {"empty-0", "empty-5", "one", "chain", "star", "twice", "mixed", "all-2", "all-12", "explicit-12"}
    for g in by.values():
        n = g["n"]
        pairs = g["pairs"] if g["listed"] else None
        assert len(g["pairs"]) == g["n_pairs"]
        if not g["listed"]:
            assert g["pairs"] == [(i, j) for i in range(n) for j in range(i + 1, n)]  # pair_at() without a list
        offsets, flat = DR.csr(n, pairs)
        level = DR.levels(n, pairs)
        first, members = DR.members_by_level(level)
        assert (g["O"], g["N"], g["V"], g["F"], g["M"]) == (offsets, flat, level, first, members), g["name"]
        assert list(delay_levels(n, pairs)) == level
    assert by["empty-0"]["V"] == [] and by["empty-0"]["F"] == [0] and by["empty-5"]["V"] == [0] * 5 and by["empty-5"]["F"] == [0, 5]
    assert by["chain"]["V"] == list(range(7)) and by["star"]["V"] == [0, 1, 1, 1, 1, 1] and by["star"]["F"] == [0, 1, 6]
    assert by["twice"]["N"] == [0, 0, 0, 1, 1, 1, 2] and by["twice"]["V"] == [0, 1, 2, 3]  # a pair given twice is listed twice, and changes no level
    assert by["all-12"]["V"] == list(range(12)) and all(by["all-12"][k] == by["explicit-12"][k] for k in "ONVFM")
