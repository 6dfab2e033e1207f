"""CPU side of the timetable look-ups (pp_pipeline_timetable / pp_planner_timetable; k_timetable_tickets in pathplanning_amd/csrc/pp_timetable.hpp):
the entries and the four records are declared, exported and mirrored in ctypes offset for offset (16 / 40 / 32 / 128 bytes), the kernel's text leaves
the rule to pp_timetable_rule.hpp and has no atomic and no inline assembly, and the Python layers, the C++ mirror and the pybind11 module expose the
call (no GPU needed)."""
import ctypes as C
import importlib
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = [("by", C.c_int32, 0), ("max_stops", C.c_int32, 4), ("reserved", C.c_int32 * 2, 8)]
PLAN = [("status", C.c_int32, 0), ("n_samples", C.c_int32, 4), ("n_stops", C.c_int32, 8), ("n_listed", C.c_int32, 12), ("s_first", C.c_double, 16), ("s_last", C.c_double, 24),
        ("duration", C.c_double, 32)]
STOP = [("row", C.c_int32, 0), ("reserved", C.c_int32, 4), ("s", C.c_double, 8), ("t_arrive", C.c_double, 16), ("t_depart", C.c_double, 24)]
RESULT = [("status", C.c_int32, 0), ("row", C.c_int32, 4), ("edge", C.c_int32, 8), ("direction", C.c_int32, 12), ("s", C.c_double, 16), ("t", C.c_double, 24), ("v", C.c_double, 32),
          ("a", C.c_double, 40), ("ratio", C.c_double, 48), ("kappa", C.c_double, 56), ("pose", C.c_double * 3, 64), ("next_stop", C.c_int32, 88), ("reserved", C.c_int32, 92),
          ("s_to_stop", C.c_double, 96), ("t_to_stop", C.c_double, 104), ("t_remaining", C.c_double, 112), ("reserved1", C.c_double, 120)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import TimetableParams, TimetablePlan, TimetableResult, TimetableStop
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_timetable_params\s*\{\s*int32_t\s+by\s*;\s*int32_t\s+max_stops\s*;\s*int32_t\s+reserved\[2\]\s*;\s*\}\s*pp_timetable_params\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_timetable_plan\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+n_samples\s*;\s*int32_t\s+n_stops\s*;\s*int32_t\s+n_listed\s*;"
                     r"\s*double\s+s_first\s*,\s*s_last\s*,\s*duration\s*;\s*\}\s*pp_timetable_plan\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_timetable_stop\s*\{\s*int32_t\s+row\s*;\s*int32_t\s+reserved\s*;\s*double\s+s\s*,\s*t_arrive\s*,\s*t_depart\s*;\s*\}\s*pp_timetable_stop\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_timetable_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+row\s*;\s*int32_t\s+edge\s*;\s*int32_t\s+direction\s*;\s*double\s+s\s*,\s*t\s*,\s*v\s*,\s*a\s*;"
                     r"\s*double\s+ratio\s*,\s*kappa\s*;\s*double\s+pose\[3\]\s*;\s*int32_t\s+next_stop\s*;\s*int32_t\s+reserved\s*;\s*double\s+s_to_stop\s*,\s*t_to_stop\s*;"
                     r"\s*double\s+t_remaining\s*;\s*double\s+reserved1\s*;\s*\}\s*pp_timetable_result\s*;", txt)
    tail = (r"\s*int32_t\s+n_points\s*,\s*const\s+double\s*\*\s*values_host\s*,\s*const\s+pp_timetable_params\s*\*\s*params\s*,\s*pp_timetable_plan\s*\*\s*plans_host\s*,"
            r"\s*pp_timetable_stop\s*\*\s*stops_host\s*,\s*pp_timetable_result\s*\*\s*results_host\s*\)\s*;")
    assert re.search(r"\bint\s+pp_pipeline_timetable\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*," + tail, txt)
    assert re.search(r"\bint\s+pp_planner_timetable\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*int32_t\s+n_queries\s*," + tail, txt)
    whole = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert "timetable look-ups and stops" in whole and "the listed ones are searched" in whole and "departure side" in whole
    assert whole.index("the pairs that can meet, by a space-time broad phase") < whole.index("timetable look-ups and stops")
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_timetable") and hasattr(lib, "pp_planner_timetable")
    # the ctypes records are the C ones, field for field and offset for offset: 16, 40, 32 and 128 bytes
    for cls, fields, size in ((TimetableParams, PARAMS, 16), (TimetablePlan, PLAN, 40), (TimetableStop, STOP, 32), (TimetableResult, RESULT, 128)):
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields]
        for n, t, off in fields:
            mine = dict(cls._fields_)[n]
            assert mine is t or (mine._length_ == t._length_ and mine._type_ is t._type_), n
            assert getattr(cls, n).offset == off, (cls.__name__, n)
        assert C.sizeof(cls) == size
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_timetable.hpp")).read()
    for name, size in (("pp_timetable_params", 16), ("pp_timetable_plan", 40), ("pp_timetable_stop", 32), ("pp_timetable_result", 128)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in kernel
    from pathplanning_amd import planner
    assert planner.TIMETABLE_PLAN_DTYPE.itemsize == 40 and planner.TIMETABLE_STOP_DTYPE.itemsize == 32 and planner.TIMETABLE_DTYPE.itemsize == 128
    for dtype, fields in ((planner.TIMETABLE_PLAN_DTYPE, PLAN), (planner.TIMETABLE_STOP_DTYPE, STOP), (planner.TIMETABLE_DTYPE, RESULT)):
        assert [(n, dtype.fields[n][1]) for n in dtype.names] == [(n, off) for n, _, off in fields]


def test_the_kernels_text_leaves_the_rule_to_the_rule():
    csrc = os.path.join(ROOT, "pathplanning_amd", "csrc")
    kernel = open(os.path.join(csrc, "pp_timetable.hpp")).read()
    for name in ("k_timetable_tickets", "ppm::is_stop", "ppm::arrive_time", "ppm::at_time", "ppm::at_length", "ppm::next_stop", "ppl::edge_of", "ppl::ratio_of", "load_edge(",
                 ".interpolate(", ".direction(", ".curvature(", "__ballot", "__popcll", "__threadfence_block", "__syncthreads"):
        assert name in kernel, name
    code = re.sub(r"//.*", "", kernel)
    assert "atomic" not in code.lower() and "asm" not in code and "sqrt" not in code
    assert code.index("__threadfence_block") < code.index("ppm::at_time") and code.index("ppm::arrive_time") < code.index("__threadfence_block")
    rule = open(os.path.join(csrc, "pp_timetable_rule.hpp")).read()
    assert "PPM_INLINE" in rule and "__host__ __device__" in rule and "namespace ppm" in rule
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", rule) == ["cstddef", "cstdint", "pp_conflict_rule.hpp"]
    plain = re.sub(r"//.*", "", rule)
    assert not re.search(r"\b(std::|malloc|new |memcpy|memset|sort|float)\b", plain) and not re.search(r"(?<!__builtin_)\b(sin|cos|exp|log|pow|hypot|fmin|fmax|sqrt)\s*\(", plain)
    for name in ("is_stop(", "arrive_time(", "row_of_length(", "step_speed(", "step_inverse(", "at_time(", "at_length(", "next_stop(", "ppc::row_of", "ppc::step_position", "ppv::step_time"):
        assert name in rule, name
    src = open(os.path.join(csrc, "pp_planner.hip")).read()
    assert src.index('#include "pp_pairs.hpp"') < src.index('#include "pp_timetable.hpp"') and '#include "pp_timetable_rule.hpp"' in src
    assert "int timetable_plans(const HeldPlans& h" in src and src.index("int candidate_pairs_plans(") < src.index("int timetable_plans(")
    held = open(os.path.join(csrc, "pp_held_plans.hpp")).read()
    assert "struct TimetableGroup" in held and "held_grow(h, g.lookups" in src and "held_grow(h, g.listed" in src and "held_run(" in src[src.index("int timetable_plans("):]
    # the kernels of the calls whose rows and readers it shares live in their own files, which know nothing of it
    for name in ("pp_conflicts.hpp", "pp_speed_profile.hpp", "pp_conflict_rule.hpp", "pp_speed_rule.hpp", "pp_locate_rule.hpp"):
        text = open(os.path.join(csrc, name)).read()
        assert "ppm::" not in text and "k_timetable_tickets" not in text, name


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.timetable)
    assert list(sig.parameters) == ["self", "tickets", "values", "by", "max_stops"]
    assert [sig.parameters[k].default for k in ("by", "max_stops")] == ["length", 16]
    sig = inspect.signature(planner.HybridAStarBatch.timetable)
    assert list(sig.parameters) == ["self", "values", "n_queries", "by", "max_stops"]
    assert [sig.parameters[k].default for k in ("n_queries", "by", "max_stops")] == [None, "length", 16]


def test_pyplanning_binds_timetable():
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.timetable)
    doc = nav.HybridAStarPipeline.timetable.__doc__
    assert all(w in doc for w in ["tickets", "values", "by", "max_stops", "speed_profile", "t_arrive", "next_stop", "t_remaining"])


def test_the_cpp_mirror_test_program_compiles_and_links():
    """tests/cpp/test_pipeline_timetable.cpp (run by the GPU suite) builds against the C++ mirror: Timetable and its records exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_timetable_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"std::vector<Timetabled>\s+Timetable\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*const\s+std::vector<std::vector<double>>&\s*values\s*,", hpp)
    assert "struct Timetabled" in hpp and "pp_pipeline_timetable(" in hpp
    assert "b.build_pipeline_timetable_test()" in open(os.path.join(ROOT, "__graft_entry__.py")).read() and "b.build_timetable_rule_test()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
