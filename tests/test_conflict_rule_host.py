"""CPU: the arithmetic of a conflict call (pathplanning_amd/csrc/pp_conflict_rule.hpp, the text k_trajectory_tickets and k_conflict_pairs compile for
the device) run by tests/cpp/test_conflict_rule.cpp -- a stand-alone program with its own main, built with g++ without contraction under the address
and undefined-behaviour sanitizers and run as a child process.  Nothing loaded into this interpreter runs under a sanitizer.

The program checks itself (see its head).  It also prints what it computed as hex floats, so every double arrives bit for bit, and this file compares
every printed value with tests/conflict_restatement.py -- the numpy restatement the GPU tests compare the kernels with -- EXACTLY."""
import subprocess

import numpy as np

import conflict_restatement as CR


def run_program():
    from pathplanning_amd import build
    exe = build.build_conflict_rule_test(verbose=False)
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


def profiles():
    out, cur = [], None
    for ln in program():
        if ln[0] == "Q":
            cur = dict(name=ln[1], n=int(ln[2]), a_acc=f(ln[3]), a_dec=f(ln[4]), rows=[], asked=[])
            out.append(cur)
        elif ln[0] == "R":
            cur["rows"].append([f(x) for x in ln[1:4]])
        elif ln[0] == "U":
            cur["asked"].append((f(ln[1]), int(ln[2]), int(ln[3]), int(ln[4]), f(ln[5])))
    return out


def test_the_program_checks_itself_and_ends_clean():
    assert program()[-1] == ["conflict", "rule", "ok"]


def test_positions_equal_the_restatement_bit_for_bit():
    names, asked = [], 0
    for q in profiles():
        rows = np.array(q["rows"])
        assert len(rows) == q["n"]
        names.append(q["name"])
        got = np.array(q["asked"])
        for hb in (0, 1):
            for ha in (0, 1):
                k = (got[:, 1] == hb) & (got[:, 2] == ha)
                if not k.any():
                    continue
                present, s = CR.position(rows, got[k, 0], q["a_acc"], q["a_dec"], hb, ha)
                assert np.array_equal(present, got[k, 3] != 0), (q["name"], hb, ha)
                # (an absent vehicle's arc length is printed too: the end it is absent beyond)
                bad = np.flatnonzero(bits(s) != bits(got[k, 4]))
                assert len(bad) == 0, (q["name"], hb, ha, got[k][bad[0]], s[bad[0]])
                asked += int(k.sum())
    for need in ("rest-to-rest", "junction-cusp-dwell", "two-standing", "standing-dwell-standing", "one", "one-at-zero", "all-at-one-place", "random-11"):
        assert need in names, need
    assert asked > 150000
    # what the hand-made ones are for
    by = {q["name"]: q for q in profiles()}
    cusp = np.array(by["junction-cusp-dwell"]["rows"])
    assert (np.diff(cusp[:, 0]) == 0.0).sum() == 2 and abs((cusp[6, 2] - cusp[5, 2]) - 1.25) < 1e-12  # a junction, and a cusp stop that dwells 1.25 s
    inside = [(u, s) for u, hb, ha, present, s in by["junction-cusp-dwell"]["asked"] if cusp[5, 2] < u < cusp[6, 2]]
    assert len(inside) > 100 and all(s == 2.0 for _, s in inside)  # the trajectory stands for the dwell
    two = np.array(by["two-standing"]["rows"])
    assert two[1, 2] > 2.0 and two[0, 1] == 0.0 and two[1, 1] == 0.0
    assert len(by["one"]["rows"]) == 1 and {(hb, ha, present) for u, hb, ha, present, s in by["one"]["asked"] if u < 0} == {(0, 0, 0), (0, 1, 0), (1, 0, 1), (1, 1, 1)}
    assert {(hb, ha, present) for u, hb, ha, present, s in by["one"]["asked"] if u > 0} == {(0, 0, 0), (0, 1, 1), (1, 0, 0), (1, 1, 1)}


def test_the_lattice_equals_the_restatement():
    lines = [ln for ln in program() if ln[0] == "L"]
    assert len(lines) >= 50
    seen = set()
    for ln in lines:
        t_from, t_to, dt, k0, T = f(ln[1]), f(ln[2]), f(ln[3]), int(ln[4]), int(ln[5])
        mine_k0, mine_T = CR.lattice(t_from, t_to, dt)
        assert mine_k0 == k0 and min(mine_T, CR.MAX_TIMES + 1) == T, ln
        if 1 <= T <= CR.MAX_TIMES:
            tau = CR.times(k0, T, dt) if T <= 5000 else np.array([float(k0), float(k0 + T - 1)]) * dt
            assert bits(tau[0]) == bits(f(ln[6])) and bits(tau[-1]) == bits(f(ln[7])), ln
        seen.add("none" if T == 0 else "too many" if T > CR.MAX_TIMES else "one" if T == 1 else "negative" if k0 < 0 else "some")
    assert seen == {"none", "too many", "one", "negative", "some"}
    assert CR.lattice(0.0, 60.0, 0.1) == (0, 601) and CR.lattice(-1.05, 1.05, 0.1) == (-10, 21) and CR.lattice(0.5, 0.5, 0.25) == (2, 1) and CR.lattice(0.55, 0.55, 0.25)[1] == 0


def test_separations_orders_and_pairs_equal_the_definition():
    lines = program()
    seps = [ln for ln in lines if ln[0] == "S"]
    assert len(seps) >= 66
    for ln in seps:
        dx, dy, ra, rb, got, margin = (f(x) for x in ln[1:7])
        with np.errstate(over="ignore", under="ignore"):
            want = np.sqrt(dx * dx + dy * dy) - (ra + rb)
        assert bits(want) == bits(got) and int(ln[7]) == int(want < margin), ln
    # the whole pair record through the restatement on two one-point trajectories gives the same separation
    ln = seps[0]
    one = lambda x, y: dict(status=0, present=np.ones(1, dtype=bool), poses=np.array([[x, y, 0.0]]), s=np.zeros(1), decided=np.ones(1, dtype=bool))
    rec = CR.pair(one(float(f(ln[1])), float(f(ln[2]))), one(0.0, 0.0), np.zeros(1), [(0.0, 0.0, 1.25)], 0.0)
    assert rec["min_separation"] == 5.0 - 2.5 and rec["status"] == 0
    orders = [ln for ln in lines if ln[0] == "O"]
    assert len(orders) == 8
    for ln in orders:
        sep, tau, best, tau_best = (f(x) for x in ln[1:5])
        assert int(ln[5]) == int(sep < best or (sep == best and tau < tau_best)) and int(ln[6]) == int(tau < tau_best), ln
    pairs = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "I"]
    assert len(pairs) >= 31 + 48  # (every pair of 2, 3, 4 and 7 plans; every 997th of 48, 64 and 301)
    for n in sorted({p[0] for p in pairs}):
        every = CR.all_pairs(n)
        for _, p, i, j in (x for x in pairs if x[0] == n):
            assert every[p] == (i, j)
