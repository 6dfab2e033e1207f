"""CPU side of the re-validation of held plans against a changed map (pp_pipeline_revalidate / pp_planner_revalidate,
k_revalidate_tickets in pathplanning_amd/csrc/pp_revalidate.hpp): the entries and the result record are declared and exported, the kernel
is in the built code object within the planner's headroom as one wave per workgroup, and the Python layers and the pybind11 module expose
the call (no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_record_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import RevalidateResult
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_revalidate_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+n_edges\s*;\s*int32_t\s+blocked_edge\s*;\s*float\s+blocked_ratio\s*;"
                     r"\s*double\s+valid_length\s*;\s*double\s+length\s*;\s*\}\s*pp_revalidate_result\s*;", txt)
    assert re.search(r"\bint\s+pp_pipeline_revalidate\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*pp_map\s*\*\s*target\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,"
                     r"\s*pp_revalidate_result\s*\*\s*results_host\s*\)\s*;", txt)
    assert re.search(r"\bint\s+pp_planner_revalidate\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*pp_map\s*\*\s*target\s*,\s*int32_t\s+n_queries\s*,"
                     r"\s*pp_revalidate_result\s*\*\s*results_host\s*\)\s*;", txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_revalidate") and hasattr(lib, "pp_planner_revalidate")
    # the ctypes record is the C one: 3 x int32, float, 2 x double
    assert [(n, t) for n, t in RevalidateResult._fields_] == [("status", C.c_int32), ("n_edges", C.c_int32), ("blocked_edge", C.c_int32), ("blocked_ratio", C.c_float),
                                                             ("valid_length", C.c_double), ("length", C.c_double)]
    assert C.sizeof(RevalidateResult) == 32


def test_the_kernel_is_built_as_one_wave_within_the_planner_headroom():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    assert "k_revalidate_tickets" in res, sorted(res)
    k = res["k_revalidate_tickets"]
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    assert k["scratch_bytes_per_lane"] <= reserve, k
    assert k["max_flat_workgroup_size"] == 64, k
    assert '#include "pp_revalidate.hpp"' in src


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    assert list(inspect.signature(planner.HybridAStarPipeline.revalidate).parameters) == ["self", "tickets", "map_set"]
    assert list(inspect.signature(planner.HybridAStarBatch.revalidate).parameters) == ["self", "n_queries", "map_set"]
    assert inspect.signature(planner.HybridAStarPipeline.revalidate).parameters["map_set"].default is None
    assert inspect.signature(planner.HybridAStarBatch.revalidate).parameters["n_queries"].default is None
    assert inspect.signature(planner.HybridAStarBatch.revalidate).parameters["map_set"].default is None


def test_pyplanning_binds_revalidate():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.revalidate)
    assert "tickets" in nav.HybridAStarPipeline.revalidate.__doc__ and "validator" in nav.HybridAStarPipeline.revalidate.__doc__


def test_the_cpp_mirror_test_program_compiles():
    """tests/cpp/test_pipeline_revalidate.cpp (run by the GPU suite) builds against the C++ mirror: Revalidate and its record exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_revalidate_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"std::vector<Revalidation>\s+Revalidate\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,", hpp)
