"""CPU side of the space-time broad phase (pp_pipeline_candidate_pairs / pp_planner_candidate_pairs; k_plan_boxes, k_box_pairs and k_pair_offsets in
pathplanning_amd/csrc/pp_pairs.hpp): the entries and both records are declared, exported and mirrored in ctypes offset for offset, the kernels' text
leaves the rule to pp_pair_rule.hpp and has no atomic, the files of the calls it serves are as they were, and the Python layers, the C++ mirror and the
pybind11 module expose the call (no GPU needed)."""
import ctypes as C
import importlib
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = [("delay", None, 0), ("times_per_box", C.c_int32, 48), ("max_pairs", C.c_int32, 52)]
SUMMARY = [("n_found", C.c_int64, 0), ("n_written", C.c_int32, 8), ("n_boxes", C.c_int32, 12), ("reach", C.c_double, 16), ("n_boxed", C.c_int32, 24), ("reserved", C.c_int32, 28)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import DelayParams, PairParams, PairSummary
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_pair_params\s*\{\s*pp_delay_params\s+delay\s*;\s*int32_t\s+times_per_box\s*;\s*int32_t\s+max_pairs\s*;\s*\}\s*pp_pair_params\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_pair_summary\s*\{\s*int64_t\s+n_found\s*;\s*int32_t\s+n_written\s*;\s*int32_t\s+n_boxes\s*;\s*double\s+reach\s*;\s*int32_t\s+n_boxed\s*;"
                     r"\s*int32_t\s+reserved\s*;\s*\}\s*pp_pair_summary\s*;", txt)
    tail = (r"\s*const\s+pp_pair_params\s*\*\s*params\s*,\s*int32_t\s*\*\s*pairs_host\s*,\s*int32_t\s*\*\s*first_box_host\s*,\s*double\s*\*\s*boxes_host\s*,"
            r"\s*pp_pair_summary\s*\*\s*summary\s*\)\s*;")
    assert re.search(r"\bint\s+pp_pipeline_candidate_pairs\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    assert re.search(r"\bint\s+pp_planner_candidate_pairs\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*int32_t\s+n_queries\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    whole = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert "the pairs that can meet" in whole and "Guarantee." in whole and "10^6 m" in whole
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_candidate_pairs") and hasattr(lib, "pp_planner_candidate_pairs")
    # the ctypes records are the C ones, field for field and offset for offset: 56 and 32 bytes
    for cls, fields in ((PairParams, PARAMS), (PairSummary, SUMMARY)):
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields]
        for n, t, off in fields:
            assert dict(cls._fields_)[n] is (t or DelayParams) and getattr(cls, n).offset == off, n
    assert C.sizeof(PairParams) == 56 and C.sizeof(PairSummary) == 32 and C.sizeof(DelayParams) == 48
    kernels = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_pairs.hpp")).read()
    assert "static_assert(sizeof(pp_pair_params) == 56" in kernels and "static_assert(sizeof(pp_pair_summary) == 32" in kernels


def test_the_kernels_text_leaves_the_rule_to_the_rule_and_the_earlier_calls_files_are_as_they_were():
    csrc = os.path.join(ROOT, "pathplanning_amd", "csrc")
    kernels = open(os.path.join(csrc, "pp_pairs.hpp")).read()
    for name in ("k_plan_boxes", "k_box_pairs", "k_pair_offsets", "template <bool Fill>", "ppb::first_column", "ppb::last_column", "ppb::accumulate", "ppb::merge", "ppb::can_meet",
                 "ppb::no_box", "ppb::exists", "__shfl_xor", "__shfl_up", "__ballot", "__popcll"):
        assert name in kernels, name
    code = re.sub(r"//.*", "", kernels)
    # the order is part of the result: no atomic on an output cursor, no shared memory, no barrier, no inline assembly
    assert "atomic" not in code.lower() and "asm" not in code and "__syncthreads" not in code and "__shared__" not in code and "while" not in code and "sqrt" not in code
    rule = open(os.path.join(csrc, "pp_pair_rule.hpp")).read()
    assert "PPB_INLINE" in rule and "__host__ __device__" in rule and "namespace ppb" in rule
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", rule) == ["cstddef", "cstdint"]  # no library function but the builtin square root
    assert not re.search(r"\b(std::|malloc|new |memcpy|memset|sort|float)\b", re.sub(r"//.*", "", rule))
    for name in ("box_count(", "first_column(", "last_column(", "disc_reach(", "reach(", "merge(", "accumulate(", "gap(", "can_meet("):
        assert name in rule, name
    src = open(os.path.join(csrc, "pp_planner.hip")).read()
    assert src.index('#include "pp_deconflict.hpp"') < src.index('#include "pp_pairs.hpp"') and '#include "pp_pair_rule.hpp"' in src
    assert "int candidate_pairs_plans(const HeldPlans& h" in src and src.index("int deconflict_plans(") < src.index("int candidate_pairs_plans(")
    held = open(os.path.join(csrc, "pp_held_plans.hpp")).read()
    assert "struct PairGroup" in held and "held_grow(h, g.doubles" in src and "held_grow(h, g.listed" in src
    # the kernels of the calls the list feeds live in their own files, which know nothing of boxes
    for name in ("pp_conflicts.hpp", "pp_deconflict.hpp", "pp_tracks.hpp", "pp_delay_rule.hpp", "pp_conflict_rule.hpp", "pp_track_rule.hpp"):
        text = open(os.path.join(csrc, name)).read()
        assert "ppb::" not in text and "k_box_pairs" not in text and "k_plan_boxes" not in text, name


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.candidate_pairs)
    assert list(sig.parameters) == ["self", "tickets", "t_start", "times_per_box", "max_delay_steps", "boxes", "max_pairs", "lattice"]
    assert [sig.parameters[k].default for k in ("times_per_box", "max_delay_steps", "boxes", "max_pairs")] == [64, 0, False, None]
    assert sig.parameters["lattice"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(planner.HybridAStarBatch.candidate_pairs)
    assert list(sig.parameters) == ["self", "t_start", "n_queries", "times_per_box", "max_delay_steps", "boxes", "max_pairs", "lattice"]
    # the boxes a call over a lattice has, as the wrapper sizes them
    assert planner._box_count(0.0, 60.0, 0.1, 64) == 10 and planner._box_count(0.0, 60.0, 0.1, 601) == 1 and planner._box_count(0.0, 60.0, 0.1, 1) == 601
    assert planner._box_count(0.7 - 1e-9, 0.75, 0.1, 16) == 1 and planner._box_count(1.0, 0.0, 0.1, 16) == 1 and planner._box_count(0.0, 1.0, 0.0, 16) == 1


def test_pyplanning_binds_candidate_pairs():
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.candidate_pairs)
    doc = nav.HybridAStarPipeline.candidate_pairs.__doc__
    assert all(w in doc for w in ["tickets", "t_start", "times_per_box", "max_delay_steps", "boxes", "max_pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after"])


def test_the_cpp_mirror_test_program_compiles_and_links():
    """tests/cpp/test_pipeline_candidate_pairs.cpp (run by the GPU suite) builds against the C++ mirror: CandidatePairs and its record exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_candidate_pairs_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"Candidates\s+CandidatePairs\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*const\s+std::vector<double>&\s*tStart\s*,\s*const\s+ConflictHorizon&\s*horizon\s*,", hpp)
    assert "struct Candidates" in hpp and "pp_pipeline_candidate_pairs(" in hpp
