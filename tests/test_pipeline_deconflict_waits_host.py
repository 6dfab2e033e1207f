"""CPU side of waits at stops that clear conflicts between held plans (pp_pipeline_deconflict_waits / pp_planner_deconflict_waits, k_wait_places and
k_wait_level in pathplanning_amd/csrc/pp_waits.hpp): the entries and the four records are declared, exported and mirrored in ctypes offset for offset,
the Python layers check their own arguments, and the C++ mirror and the pybind11 module expose the call (no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESULT = [("status", C.c_int32, 0), ("place", C.c_int32, 4), ("row", C.c_int32, 8), ("wait_steps", C.c_int32, 12), ("n_tried", C.c_int32, 16), ("blocker", C.c_int32, 20),
          ("t_start", C.c_double, 24), ("t_hold", C.c_double, 32), ("t_resume", C.c_double, 40), ("s_wait", C.c_double, 48), ("t_block", C.c_double, 56), ("s_block", C.c_double * 2, 64)]
PLACE = [("row", C.c_int32, 0), ("column", C.c_int32, 4), ("s", C.c_double, 8), ("t_arrive", C.c_double, 16), ("pose", C.c_double * 3, 24), ("sin_theta", C.c_double, 48),
         ("cos_theta", C.c_double, 56)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import DelayParams, WaitFixed, WaitParams, WaitPlace, WaitResult
    from pathplanning_amd.planner import WAIT_DTYPE, WAIT_FIXED_DTYPE, WAIT_PLACE_DTYPE
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_wait_params\s*\{\s*pp_delay_params\s+delay\s*;\s*int32_t\s+max_places\s*;\s*int32_t\s+reserved\s*;\s*\}\s*pp_wait_params\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_wait_fixed\s*\{\s*int32_t\s+row\s*;\s*int32_t\s+steps\s*;\s*\}\s*pp_wait_fixed\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_wait_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+place\s*;\s*int32_t\s+row\s*;\s*int32_t\s+wait_steps\s*;\s*int32_t\s+n_tried\s*;"
                     r"\s*int32_t\s+blocker\s*;\s*double\s+t_start\s*;\s*double\s+t_hold\s*;\s*double\s+t_resume\s*;\s*double\s+s_wait\s*;\s*double\s+t_block\s*;"
                     r"\s*double\s+s_block\[2\]\s*;\s*\}\s*pp_wait_result\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_wait_place\s*\{\s*int32_t\s+row\s*,\s*column\s*;\s*double\s+s\s*,\s*t_arrive\s*;\s*double\s+pose\[3\]\s*;\s*double\s+sin_theta\s*,"
                     r"\s*cos_theta\s*;\s*\}\s*pp_wait_place\s*;", txt)
    tail = (r"\s*const\s+uint8_t\s*\*\s*no_start_wait\s*,\s*const\s+pp_wait_fixed\s*\*\s*fixed\s*,\s*int32_t\s+n_pairs\s*,\s*const\s+int32_t\s*\*\s*pairs\s*,"
            r"\s*const\s+pp_wait_params\s*\*\s*params\s*,\s*int32_t\s*\*\s*n_places_host\s*,\s*pp_wait_place\s*\*\s*places_host\s*,\s*pp_wait_result\s*\*\s*results_host\s*\)\s*;")
    assert re.search(r"\bint\s+pp_pipeline_deconflict_waits\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    assert re.search(r"\bint\s+pp_planner_deconflict_waits\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*int32_t\s+n_queries\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_deconflict_waits") and hasattr(lib, "pp_planner_deconflict_waits")
    # the ctypes records are the C ones, field for field and offset for offset
    assert [n for n, _ in WaitParams._fields_] == ["delay", "max_places", "reserved"] and dict(WaitParams._fields_)["delay"] is DelayParams
    assert (WaitParams.delay.offset, WaitParams.max_places.offset, WaitParams.reserved.offset) == (0, 48, 52)
    assert WaitFixed._fields_ == [("row", C.c_int32), ("steps", C.c_int32)]
    for cls, fields, dtype in ((WaitResult, RESULT, WAIT_DTYPE), (WaitPlace, PLACE, WAIT_PLACE_DTYPE)):
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields]
        for n, t, off in fields:
            assert dict(cls._fields_)[n] is t or dict(cls._fields_)[n]._length_ == t._length_, n
            assert getattr(cls, n).offset == off, n
        # ... the numpy record the wrappers return is the same record
        assert [(n, dtype.fields[n][1]) for n in dtype.names] == [(n, off) for n, _, off in fields]
    assert (C.sizeof(WaitParams), C.sizeof(WaitFixed), C.sizeof(WaitResult), C.sizeof(WaitPlace)) == (56, 8, 80, 64)
    assert (WAIT_DTYPE.itemsize, WAIT_PLACE_DTYPE.itemsize, WAIT_FIXED_DTYPE.itemsize) == (80, 64, 8)
    # ... and the library's own view of the sizes
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_waits.hpp")).read()
    for name, size in (("pp_wait_params", 56), ("pp_wait_fixed", 8), ("pp_wait_result", 80), ("pp_wait_place", 64)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in kernel
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    held = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_held_plans.hpp")).read()
    pipe = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_pipeline.hpp")).read()
    assert "struct WaitGroup" in held and "WaitGroup wait;" in src and "WaitGroup wait;" in pipe and "held_grow(h, w.vehicles" in src and "held_grow(h, w.listed" in src
    assert src.index('#include "pp_timetable.hpp"') < src.index('#include "pp_waits.hpp"') and '#include "pp_wait_rule.hpp"' in src


def test_the_python_wrappers_have_the_calls_and_check_their_arguments():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.deconflict_waits)
    assert list(sig.parameters) == ["self", "tickets", "t_start", "pairs", "no_start_wait", "fixed", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after",
                                    "max_delay_steps", "max_places", "places"]
    assert [sig.parameters[k].default for k in ("pairs", "no_start_wait", "fixed", "t_from", "dt", "margin", "hold_before", "hold_after", "max_delay_steps", "max_places",
                                                "places")] == [None, None, None, 0.0, 0.1, 0.0, False, False, 0, 0, False]
    assert sig.parameters["t_to"].default == inspect.signature(planner.HybridAStarPipeline.deconflict).parameters["t_to"].default
    sig = inspect.signature(planner.HybridAStarBatch.deconflict_waits)
    assert list(sig.parameters)[:6] == ["self", "t_start", "n_queries", "pairs", "no_start_wait", "fixed"]
    # the committed waits: None, rows of (row, steps), the dtype itself, or an earlier call's records
    assert planner.wait_fixed(None, 3) is None
    rows = planner.wait_fixed([(-2, 0), (-1, 4), (7, 2)], 3)
    assert rows.dtype == planner.WAIT_FIXED_DTYPE and list(rows["row"]) == [-2, -1, 7] and list(rows["steps"]) == [0, 4, 2]
    assert planner.wait_fixed(rows, 3) is not None and planner.wait_fixed(rows, 3).tobytes() == rows.tobytes()
    recs = np.zeros(5, dtype=planner.WAIT_DTYPE)
    recs["status"], recs["place"], recs["row"], recs["wait_steps"] = [0, 0, 0, 1, 2], [-2, -1, 1, -2, 0], [-1, -1, 9, -1, 5], [0, 3, 2, -1, 6]
    back = planner.wait_fixed(recs.view(np.recarray), 5)
    assert list(back["row"]) == [-1, -1, 9, -2, 5] and list(back["steps"]) == [0, 3, 2, 0, 6]
    for bad in ([(-2, 0)], np.zeros(2, dtype=planner.WAIT_FIXED_DTYPE), recs[:4]):
        with pytest.raises(ValueError):
            planner.wait_fixed(bad, 3)
    with pytest.raises(ValueError):
        planner.wait_fixed([(2 ** 31, 0)], 1)


def test_pyplanning_binds_deconflict_waits():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.deconflict_waits)
    doc = nav.HybridAStarPipeline.deconflict_waits.__doc__
    assert all(w in doc for w in ["tickets", "t_start", "pairs", "no_start_wait", "fixed", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "max_delay_steps",
                                  "max_places", "speed_profile"])


def test_the_cpp_mirror_test_program_compiles():
    """tests/cpp/test_pipeline_deconflict_waits.cpp (run by the GPU suite) builds against the C++ mirror: DeconflictWaits and its records exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_deconflict_waits_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"std::vector<Wait>\s+DeconflictWaits\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*const\s+std::vector<double>&\s*tStart\s*,", hpp)
