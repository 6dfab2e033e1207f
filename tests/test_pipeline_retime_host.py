"""CPU side of the retime call (pp_pipeline_retime / pp_planner_retime; k_retime_tickets in pathplanning_amd/csrc/pp_retime.hpp): the entries and the
two records are declared, exported and mirrored in ctypes and numpy offset for offset (16 / 40 bytes), the kernel's text leaves the rule to
pp_retime_rule.hpp and has no atomic and no inline assembly, the Python layers, the C++ mirror and the pybind11 module expose the call, and
planner.wait_holds turns hand-made deconflict_waits records into holds and start times (no GPU needed)."""
import ctypes as C
import importlib
import inspect
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOLD = [("plan", C.c_int32, 0), ("row", C.c_int32, 4), ("seconds", C.c_double, 8)]
RESULT = [("status", C.c_int32, 0), ("n_holds", C.c_int32, 4), ("first_row", C.c_int32, 8), ("bad_hold", C.c_int32, 12), ("held", C.c_double, 16),
          ("duration_before", C.c_double, 24), ("duration", C.c_double, 32)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build, planner
    from pathplanning_amd._lib import Hold, RetimeResult
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_hold\s*\{\s*int32_t\s+plan\s*;\s*int32_t\s+row\s*;\s*double\s+seconds\s*;\s*\}\s*pp_hold\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_retime_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+n_holds\s*;\s*int32_t\s+first_row\s*;\s*int32_t\s+bad_hold\s*;\s*double\s+held\s*;"
                     r"\s*double\s+duration_before\s*,\s*duration\s*;\s*\}\s*pp_retime_result\s*;", txt)
    tail = r"\s*int32_t\s+n_holds\s*,\s*const\s+pp_hold\s*\*\s*holds\s*,\s*double\s*\*\s*rows_host\s*,\s*pp_retime_result\s*\*\s*results_host\s*\)\s*;"
    assert re.search(r"\bint\s+pp_pipeline_retime\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*," + tail, txt)
    assert re.search(r"\bint\s+pp_planner_retime\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*int32_t\s+n_queries\s*," + tail, txt)
    whole = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert whole.index("waits at stops that clear conflicts, by priority and ticket") < whole.index("decided waits written into the timetables, by ticket")
    for words in ("non-decreasing", "one ulp", "IN PLACE", "all or nothing", "shift", "needs no fixed entry any more and the vehicle is free again"):
        assert words in whole, words
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_retime") and hasattr(lib, "pp_planner_retime")
    for cls, fields, size in ((Hold, HOLD, 16), (RetimeResult, RESULT, 40)):
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields]
        for n, t, off in fields:
            assert dict(cls._fields_)[n] is t and getattr(cls, n).offset == off, (cls.__name__, n)
        assert C.sizeof(cls) == size
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_retime.hpp")).read()
    for name, size in (("pp_hold", 16), ("pp_retime_result", 40)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in kernel
    for dtype, fields, size in ((planner.HOLD_DTYPE, HOLD, 16), (planner.RETIME_DTYPE, RESULT, 40)):
        assert dtype.itemsize == size and [(n, dtype.fields[n][1]) for n in dtype.names] == [(n, off) for n, _, off in fields]
        assert [dtype.fields[n][0] for n in dtype.names] == [np.dtype(t) for _, t, _ in fields]


def test_the_kernels_text_leaves_the_rule_to_the_rule():
    csrc = os.path.join(ROOT, "pathplanning_amd", "csrc")
    kernel = open(os.path.join(csrc, "pp_retime.hpp")).read()
    for name in ("k_retime_tickets", "__launch_bounds__(kRetimeLanes)", "ppr::hold_status", "ppr::prefix", "ppr::hold_of", "ppr::retimed", "__ballot", "__syncthreads", "extern __shared__"):
        assert name in kernel, name
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code.lower() and "asm" not in code and "sqrt" not in code
    assert code.index("ppr::hold_status") < code.index("ppr::prefix") < code.index("__syncthreads") < code.index("ppr::retimed")
    rule = open(os.path.join(csrc, "pp_retime_rule.hpp")).read()
    assert "PPR_INLINE" in rule and "__host__ __device__" in rule and "namespace ppr" in rule
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", rule) == ["cstddef", "cstdint", "pp_timetable_rule.hpp"]
    plain = re.sub(r"//.*", "", rule)
    assert not re.search(r"\b(std::|malloc|new |memcpy|memset|sort|float)\b", plain) and not re.search(r"\b(sin|cos|exp|log|pow|hypot|fmin|fmax|sqrt)\s*\(", plain)
    for name in ("dwell(", "hold_status(", "prefix(", "hold_of(", "retimed(", "ppm::is_stop", "ppm::arrive_time"):
        assert name in rule, name
    assert "step_time" not in plain and "== 0.0" not in plain  # (it restates neither the step time nor the stop predicate)
    src = open(os.path.join(csrc, "pp_planner.hip")).read()
    assert src.index('#include "pp_timetable.hpp"') < src.index('#include "pp_retime.hpp"') and '#include "pp_retime_rule.hpp"' in src
    assert "int retime_plans(const HeldPlans& h" in src and src.index("int timetable_plans(") < src.index("int retime_plans(")
    body = src[src.index("int retime_plans("):src.index("void free_planner(")]
    assert "held_grow(h, g.plans" in body and "held_grow(h, g.listed" in body and "held_run(" in body
    held = open(os.path.join(csrc, "pp_held_plans.hpp")).read()
    assert "struct RetimeGroup" in held and "retime_plans" in held[:held.index("#pragma once")]
    before, after = held.index("struct SpeedGroup"), held.index("struct ConflictGroup")
    assert "retime" not in held[before:after].lower()  # SpeedGroup::Profile has no new field
    for name in ("pp_conflicts.hpp", "pp_speed_profile.hpp", "pp_timetable.hpp", "pp_timetable_rule.hpp", "pp_waits.hpp"):
        text = open(os.path.join(csrc, name)).read()
        assert "ppr::" not in text and "k_retime_tickets" not in text, name


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.retime)
    assert list(sig.parameters) == ["self", "tickets", "holds", "rows"] and sig.parameters["rows"].default is False
    sig = inspect.signature(planner.HybridAStarBatch.retime)
    assert list(sig.parameters) == ["self", "holds", "n_queries", "rows"]
    assert [sig.parameters[k].default for k in ("n_queries", "rows")] == [None, False]
    assert list(inspect.signature(planner.wait_holds).parameters) == ["results", "dt", "t_start"]
    holds = planner.hold_list([(0, 3, 0.5), (2, 1, -0.25)])
    assert holds.dtype == planner.HOLD_DTYPE and holds["plan"].tolist() == [0, 2] and holds["row"].tolist() == [3, 1] and holds["seconds"].tolist() == [0.5, -0.25]
    assert len(planner.hold_list(None)) == 0 and len(planner.hold_list([])) == 0 and planner.hold_list(holds) is not None


def test_wait_holds_on_hand_made_records():
    from pathplanning_amd import planner
    rec = np.zeros(8, dtype=planner.WAIT_DTYPE)
    #                status place row steps t_start (the record's effective start)
    rows = [(0, -2, -1, 0, 10.0),    # no wait
            (0, -1, -1, 4, 12.0),    # a wait at the start: the record's effective start
            (0, 1, 37, 3, 30.0),     # three steps at the stop of row 37
            (2, 0, 12, 5, 40.0),     # a fixed wait in conflict is scheduled all the same
            (1, -2, -1, -1, 50.0),   # no candidate is clear
            (-1, -2, -1, -1, 0.0),   # no profile
            (0, 0, 9, 0, 70.0),      # a place with zero steps is no wait
            (-2, 0, 5, 2, 0.0)]      # a fixed row that does not qualify
    for k, (status, place, row, steps, ts) in enumerate(rows):
        rec[k]["status"], rec[k]["place"], rec[k]["row"], rec[k]["wait_steps"], rec[k]["t_start"] = status, place, row, steps, ts
    t_start = np.array([10.0, 11.0, 30.0, 40.0, 50.0, 60.0, 70.0, 80.0])
    given = t_start.copy()
    holds, ts = planner.wait_holds(rec.view(np.recarray), 0.25, t_start)
    assert holds.dtype == planner.HOLD_DTYPE and holds["plan"].tolist() == [2, 3] and holds["row"].tolist() == [37, 12]
    assert holds["seconds"].tolist() == [3 * 0.25, 5 * 0.25]
    assert ts.tolist() == [10.0, 12.0, 30.0, 40.0, 50.0, 60.0, 70.0, 80.0] and np.array_equal(t_start, given)  # (the caller's array is not written)
    dt = 0.1
    holds, _ = planner.wait_holds(rec, dt, 0.0)  # a scalar start, a plain structured array
    assert holds["seconds"][0].tobytes() == (np.float64(3) * np.float64(dt)).tobytes()  # (double)d * dt
    assert (np.diff(holds["plan"]) > 0).all()  # ascending: what retime() takes


def test_pyplanning_binds_retime():
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.retime)
    doc = nav.HybridAStarPipeline.retime.__doc__
    assert all(w in doc for w in ["tickets", "holds", "plan", "row", "seconds", "speed_profile", "bad_hold", "duration_before"])


def test_the_cpp_mirror_has_the_call():
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"std::vector<Retimed>\s+Retime\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*const\s+std::vector<Hold>&\s*holds\s*\)", hpp)
    assert "struct Retimed" in hpp and "struct Hold" in hpp and "pp_pipeline_retime(" in hpp
    assert "b.build_retime_rule_test()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
