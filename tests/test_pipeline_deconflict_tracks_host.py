"""CPU side of start delays that clear conflicts and tracked movers (pp_pipeline_deconflict_tracks / pp_planner_deconflict_tracks; k_track_samples,
k_delay_level_tracks and k_track_pairs in pathplanning_amd/csrc/pp_tracks.hpp): the entries and both records are declared, exported and mirrored in
ctypes offset for offset, the kernels' text leaves the rule to pp_track_rule.hpp, the files of the calls it extends are as they were, and the Python
layers, the C++ mirror and the pybind11 module expose the call (no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SET = [("n_tracks", C.c_int32, 0), ("reserved", C.c_int32, 4), ("offsets", C.c_void_p, 8), ("waypoints", C.c_void_p, 16), ("radii", C.c_void_p, 24)]
RESULT = [("status", C.c_int32, 0), ("n_times", C.c_int32, 4), ("n_conflict", C.c_int32, 8), ("reserved", C.c_int32, 12), ("t_first", C.c_double, 16), ("s_first", C.c_double, 24),
          ("min_separation", C.c_double, 32), ("t_min", C.c_double, 40), ("s_min", C.c_double, 48), ("reserved1", C.c_double, 56)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import TrackResult, TrackSet
    from pathplanning_amd.planner import TRACK_DTYPE
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_track_set\s*\{\s*int32_t\s+n_tracks\s*;\s*int32_t\s+reserved\s*;\s*const\s+int32_t\s*\*\s*offsets\s*;\s*const\s+double\s*\*\s*waypoints\s*;"
                     r"\s*const\s+double\s*\*\s*radii\s*;\s*\}\s*pp_track_set\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_track_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+n_times\s*;\s*int32_t\s+n_conflict\s*;\s*int32_t\s+reserved\s*;\s*double\s+t_first\s*;"
                     r"\s*double\s+s_first\s*;\s*double\s+min_separation\s*;\s*double\s+t_min\s*;\s*double\s+s_min\s*;\s*double\s+reserved1\s*;\s*\}\s*pp_track_result\s*;", txt)
    tail = (r"\s*int32_t\s+n_pairs\s*,\s*const\s+int32_t\s*\*\s*pairs\s*,\s*const\s+pp_delay_params\s*\*\s*params\s*,\s*const\s+pp_track_set\s*\*\s*tracks\s*,"
            r"\s*pp_delay_result\s*\*\s*results_host\s*,\s*pp_track_result\s*\*\s*track_results_host\s*\)\s*;")
    assert re.search(r"\bint\s+pp_pipeline_deconflict_tracks\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    assert re.search(r"\bint\s+pp_planner_deconflict_tracks\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*int32_t\s+n_queries\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    assert "start delays that clear conflicts and tracked movers" in open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_deconflict_tracks") and hasattr(lib, "pp_planner_deconflict_tracks")
    # the ctypes records are the C ones, field for field and offset for offset: 32 and 64 bytes
    for cls, fields in ((TrackSet, SET), (TrackResult, RESULT)):
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields]
        for n, t, off in fields:
            assert dict(cls._fields_)[n] is t and getattr(cls, n).offset == off, n
    assert C.sizeof(TrackSet) == 32 and C.sizeof(TrackResult) == 64
    # ... the numpy record the wrappers return is the same record
    assert TRACK_DTYPE.itemsize == 64 and [(n, TRACK_DTYPE.fields[n][1]) for n in TRACK_DTYPE.names] == [(n, off) for n, _, off in RESULT]
    # ... and the library's own view of the sizes
    kernels = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_tracks.hpp")).read()
    assert "static_assert(sizeof(pp_track_set) == 32" in kernels and "static_assert(sizeof(pp_track_result) == 64" in kernels


def test_the_kernels_text_leaves_the_rule_to_the_rule_and_the_earlier_calls_files_are_as_they_were():
    csrc = os.path.join(ROOT, "pathplanning_amd", "csrc")
    kernels = open(os.path.join(csrc, "pp_tracks.hpp")).read()
    for name in ("k_track_samples", "k_delay_level_tracks", "k_track_pairs", "ppk::position", "ppk::key", "ppk::partner_of_track", "ppk::is_track", "ppy::column", "ppy::before",
                 "ppy::kNoKey", "ppc::separation", "ppc::in_conflict", "ppc::lattice_time", "ppc::closer", "ppc::earlier", "disc_centre(", "__shfl_xor"):
        assert name in kernels, name
    code = re.sub(r"//.*", "", kernels)
    assert "sqrt" not in code and "atomic" not in kernels.lower() and "asm" not in kernels and "__syncthreads" not in code and "__shared__" not in code and "while" not in code
    rule = open(os.path.join(csrc, "pp_track_rule.hpp")).read()
    assert "PPK_INLINE" in rule and "__host__ __device__" in rule
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", rule) == ["cstddef", "cstdint", "pp_delay_rule.hpp"]  # no library function
    assert not re.search(r"\b(std::|malloc|new |memcpy|memset|sort|sqrt|float)\b", re.sub(r"//.*", "", rule))
    for name in ("waypoint_of(", "position(", "partner_of_track(", "track_of_partner(", "validate("):
        assert name in rule, name
    src = open(os.path.join(csrc, "pp_planner.hip")).read()
    assert src.index('#include "pp_deconflict.hpp"') < src.index('#include "pp_tracks.hpp"') and '#include "pp_track_rule.hpp"' in src
    assert "int deconflict_tracks_plans(const HeldPlans& h" in src and src.index("int deconflict_plans(") < src.index("int deconflict_tracks_plans(")
    held = open(os.path.join(csrc, "pp_held_plans.hpp")).read()
    assert "struct TrackGroup" in held and "held_grow(h, t.tracks" in src and "held_grow(h, t.records" in src
    # the delay kernel and the conflict kernels live in their own files, which know nothing of tracks
    for name in ("pp_conflicts.hpp", "pp_deconflict.hpp", "pp_delay_rule.hpp", "pp_conflict_rule.hpp"):
        assert "track" not in open(os.path.join(csrc, name)).read().lower(), name


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.deconflict_tracks)
    assert list(sig.parameters) == ["self", "tickets", "t_start", "tracks", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "max_delay_steps", "details"]
    assert [sig.parameters[k].default for k in ("pairs", "t_from", "dt", "margin", "hold_before", "hold_after", "max_delay_steps", "details")] == [None, 0.0, 0.1, 0.0, False, False, 0, True]
    assert sig.parameters["t_to"].default == inspect.signature(planner.HybridAStarPipeline.deconflict).parameters["t_to"].default
    sig = inspect.signature(planner.HybridAStarBatch.deconflict_tracks)
    assert list(sig.parameters) == ["self", "t_start", "tracks", "n_queries", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "max_delay_steps", "details"]
    # the layout of a track set: offsets, rows and radii as the C ABI takes them
    tk, (offsets, rows, radii) = planner.track_set([(0.3, [(0.0, 1.0, 2.0), (1.0, 3.0, 4.0)]), (1, np.array([[5.0, 6.0, 7.0]]))])
    assert (tk.n_tracks, tk.reserved) == (2, 0) and offsets.dtype == np.int32 and list(offsets) == [0, 2, 3] and rows.shape == (3, 3) and rows.flags["C_CONTIGUOUS"]
    assert list(radii) == [0.3, 1.0] and (tk.offsets, tk.waypoints, tk.radii) == (offsets.ctypes.data, rows.ctypes.data, radii.ctypes.data)
    assert planner.track_set(None)[0].n_tracks == 0 and planner.track_set([])[0].n_tracks == 0
    for bad in (np.zeros((0, 3)), np.zeros((2, 2)), np.zeros(3)):
        try:
            planner.track_set([(1.0, bad)])
        except ValueError as e:
            assert "track 0" in str(e)
        else:
            raise AssertionError("a track without [W, 3] waypoints was accepted")


def test_pyplanning_binds_deconflict_tracks():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.deconflict_tracks)
    doc = nav.HybridAStarPipeline.deconflict_tracks.__doc__
    assert all(w in doc for w in ["tickets", "t_start", "tracks", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "max_delay_steps", "details"])


def test_the_cpp_mirror_test_program_compiles_and_links():
    """tests/cpp/test_pipeline_deconflict_tracks.cpp (run by the GPU suite) builds against the C++ mirror: DeconflictTracks and its records exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_deconflict_tracks_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"DelayedWithTracks\s+DeconflictTracks\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*const\s+std::vector<double>&\s*tStart\s*,\s*const\s+std::vector<Track>&\s*tracks\s*,", hpp)
    assert "struct TrackConflict" in hpp and "pp_pipeline_deconflict_tracks(" in hpp
