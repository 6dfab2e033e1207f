"""CPU side of stamping held plans into a map (pp_pipeline_stamp / pp_planner_stamp, k_stamp_tickets in pathplanning_amd/csrc/pp_stamp.hpp): the
entries and the records are declared and exported, the kernel is in the built code object within the planner's headroom as one wave per
workgroup, and the Python layers, the C++ mirror and the pybind11 module expose the call (no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import StampParams, StampResult
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_stamp_params\s*\{\s*double\s+spacing\s*;\s*float\s+margin\s*;\s*int32_t\s+reserved\s*;\s*\}\s*pp_stamp_params\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_stamp_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+n_samples\s*;\s*int32_t\s+cell_box\s*\[\s*4\s*\]\s*;\s*double\s+length\s*;\s*\}"
                     r"\s*pp_stamp_result\s*;", txt)
    assert re.search(r"\bint\s+pp_pipeline_stamp\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*pp_map\s*\*\s*target\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,"
                     r"\s*const\s+int32_t\s*\*\s*values\s*,\s*const\s+double\s*\*\s*from_length\s*,\s*const\s+double\s*\*\s*to_length\s*,\s*const\s+pp_stamp_params\s*\*\s*params\s*,"
                     r"\s*pp_stamp_result\s*\*\s*results_host\s*\)\s*;", txt)
    assert re.search(r"\bint\s+pp_planner_stamp\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*pp_map\s*\*\s*target\s*,\s*int32_t\s+n_queries\s*,\s*const\s+int32_t\s*\*\s*values\s*,"
                     r"\s*const\s+double\s*\*\s*from_length\s*,\s*const\s+double\s*\*\s*to_length\s*,\s*const\s+pp_stamp_params\s*\*\s*params\s*,\s*pp_stamp_result\s*\*\s*results_host\s*\)\s*;", txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_stamp") and hasattr(lib, "pp_planner_stamp")
    # the ctypes records are the C ones
    assert [(n, t) for n, t in StampParams._fields_] == [("spacing", C.c_double), ("margin", C.c_float), ("reserved", C.c_int32)]
    assert C.sizeof(StampParams) == 16
    assert [n for n, _ in StampResult._fields_] == ["status", "n_samples", "cell_box", "length"]
    assert C.sizeof(StampResult) == 32 and StampResult.length.offset == 24 and StampResult.cell_box.offset == 8


def test_the_kernel_is_built_as_one_wave_within_the_planner_headroom():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    assert "k_stamp_tickets" in res, sorted(res)
    k = res["k_stamp_tickets"]
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    assert k["scratch_bytes_per_lane"] <= reserve, k
    assert k["max_flat_workgroup_size"] == 64, k
    assert '#include "pp_stamp.hpp"' in src and '#include "pp_stamp_rule.hpp"' in src
    # the kernel and the host program share the rule: the kernel's text has no cell arithmetic of its own
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_stamp.hpp")).read()
    for name in ("pps::edge_steps", "pps::sample_ratio", "pps::sample_arc_length", "pps::in_window", "pps::axis_range", "pps::covers", "pps::effective_radius"):
        assert name in kernel, name


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.stamp)
    assert list(sig.parameters) == ["self", "tickets", "map_set", "values", "from_length", "to_length", "spacing", "margin"]
    assert [sig.parameters[k].default for k in ("map_set", "values", "from_length", "to_length")] == [None] * 4 and sig.parameters["margin"].default == 0.0
    sig = inspect.signature(planner.HybridAStarBatch.stamp)
    assert list(sig.parameters) == ["self", "n_queries", "map_set", "values", "from_length", "to_length", "spacing", "margin"]
    assert sig.parameters["n_queries"].default is None and sig.parameters["margin"].default == 0.0


def test_pyplanning_binds_stamp():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.stamp)
    doc = nav.HybridAStarPipeline.stamp.__doc__
    assert all(w in doc for w in ("tickets", "validator", "spacing", "margin", "values", "from_length", "to_length"))


def test_the_cpp_mirror_test_program_compiles():
    """tests/cpp/test_pipeline_stamp.cpp (run by the GPU suite) builds against the C++ mirror: Stamp and its record exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_stamp_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"std::vector<Stamped>\s+Stamp\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,", hpp)
