"""CPU side of locating vehicles on held plans (pp_pipeline_locate / pp_planner_locate, k_locate_tickets in pathplanning_amd/csrc/pp_locate.hpp): the
entries and the records are declared and exported, the kernel is in the built code object within the planner's headroom as one wave per
workgroup, and the Python layers, the C++ mirror and the pybind11 module expose the call (no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELDS = [("status", C.c_int32, 0), ("edge", C.c_int32, 4), ("direction", C.c_int32, 8), ("n_samples", C.c_int32, 12), ("s", C.c_double, 16), ("ratio", C.c_double, 24),
          ("distance", C.c_double, 32), ("along", C.c_double, 40), ("lateral", C.c_double, 48), ("heading_error", C.c_double, 56), ("length", C.c_double, 64)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import LocateParams, LocateResult
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_locate_params\s*\{\s*double\s+spacing\s*;\s*double\s+heading_weight\s*;\s*\}\s*pp_locate_params\s*;", txt)
    members = r"\s*".join([r"int32_t\s+%s\s*;" % n for n, t, _ in FIELDS if t is C.c_int32] + [r"double\s+%s\s*;" % n for n, t, _ in FIELDS if t is C.c_double] +
                          [r"double\s+pose\s*\[\s*3\s*\]\s*;"])
    assert re.search(r"typedef\s+struct\s+pp_locate_result\s*\{\s*" + members + r"\s*\}\s*pp_locate_result\s*;", txt)
    assert re.search(r"\bint\s+pp_pipeline_locate\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,\s*const\s+double\s*\*\s*poses_host\s*,"
                     r"\s*const\s+double\s*\*\s*from_length\s*,\s*const\s+double\s*\*\s*to_length\s*,\s*const\s+pp_locate_params\s*\*\s*params\s*,"
                     r"\s*pp_locate_result\s*\*\s*results_host\s*\)\s*;", txt)
    assert re.search(r"\bint\s+pp_planner_locate\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*int32_t\s+n_queries\s*,\s*const\s+double\s*\*\s*poses_host\s*,"
                     r"\s*const\s+double\s*\*\s*from_length\s*,\s*const\s+double\s*\*\s*to_length\s*,\s*const\s+pp_locate_params\s*\*\s*params\s*,\s*pp_locate_result\s*\*\s*results_host\s*\)\s*;", txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_locate") and hasattr(lib, "pp_planner_locate")
    # the ctypes records are the C ones
    assert [(n, t) for n, t in LocateParams._fields_] == [("spacing", C.c_double), ("heading_weight", C.c_double)]
    assert C.sizeof(LocateParams) == 16
    assert [n for n, _ in LocateResult._fields_] == [n for n, _, _ in FIELDS] + ["pose"]
    for n, t, off in FIELDS:
        assert dict(LocateResult._fields_)[n] is t and getattr(LocateResult, n).offset == off, n
    assert LocateResult.pose.offset == 72 and C.sizeof(LocateResult) == 96


def test_the_kernel_is_built_as_one_wave_within_the_planner_headroom():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    assert "k_locate_tickets" in res, sorted(res)
    k = res["k_locate_tickets"]
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    assert k["scratch_bytes_per_lane"] <= reserve, k
    assert k["max_flat_workgroup_size"] == 64, k
    assert k["vgpr_spill"] == 0 and k["lds_bytes"] == 0, k  # (its LDS is dynamic: 12 B per path-capacity entry)
    assert '#include "pp_locate.hpp"' in src and '#include "pp_locate_rule.hpp"' in src
    assert src.index('#include "pp_stamp.hpp"') < src.index('#include "pp_locate.hpp"')
    # the kernel and the host program share the rule: the kernel's text has no wrap, cost, order, lattice or edge arithmetic of its own
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_locate.hpp")).read()
    for name in ("ppl::error_of", "ppl::cost", "ppl::better", "ppl::lattice_step", "ppl::lattice_first", "ppl::lattice_point", "ppl::edge_of", "ppl::ratio_of", "ppl::names_next_edge",
                 "pps::edge_steps", "pps::sample_ratio", "pps::sample_arc_length", "pps::in_window"):
        assert name in kernel, name
    assert "rint" not in kernel and "atomic" not in kernel.lower() and "asm" not in kernel
    rule = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_locate_rule.hpp")).read()
    assert "wrap(" in rule and "pps::in_window" in rule


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.locate)
    assert list(sig.parameters) == ["self", "tickets", "poses", "from_length", "to_length", "spacing", "heading_weight"]
    assert [sig.parameters[k].default for k in ("from_length", "to_length", "spacing", "heading_weight")] == [None, None, 0.1, 0.0]
    sig = inspect.signature(planner.HybridAStarBatch.locate)
    assert list(sig.parameters) == ["self", "poses", "n_queries", "from_length", "to_length", "spacing", "heading_weight"]
    assert [sig.parameters[k].default for k in ("n_queries", "from_length", "to_length", "spacing", "heading_weight")] == [None, None, None, 0.1, 0.0]


def test_pyplanning_binds_locate():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.locate)
    doc = nav.HybridAStarPipeline.locate.__doc__
    assert all(w in doc for w in ("tickets", "poses", "spacing", "heading_weight", "from_length", "to_length"))


def test_the_cpp_mirror_test_program_compiles():
    """tests/cpp/test_pipeline_locate.cpp (run by the GPU suite) builds against the C++ mirror: Locate and its record exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_locate_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"std::vector<Located>\s+Locate\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*const\s+std::vector<Pose2d>&\s*poses\s*,", hpp)
