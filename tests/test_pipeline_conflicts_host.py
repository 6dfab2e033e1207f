"""CPU side of space-time conflicts between held plans (pp_pipeline_conflicts / pp_planner_conflicts, k_trajectory_tickets and k_conflict_pairs in
pathplanning_amd/csrc/pp_conflicts.hpp): the entries and the three records are declared, exported and mirrored in ctypes offset for offset, both
kernels are in the built code object as one wave per workgroup within the resource figures DESIGN.md 4.10 records, their text leaves the arithmetic
to the shared rule, and the Python layers, the C++ mirror and the pybind11 module expose the call (no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PARAMS = [("t_from", C.c_double, 0), ("t_to", C.c_double, 8), ("dt", C.c_double, 16), ("margin", C.c_double, 24), ("hold_before", C.c_int32, 32), ("hold_after", C.c_int32, 36)]
PLAN = [("status", C.c_int32, 0), ("n_present", C.c_int32, 4), ("first", C.c_int32, 8), ("last", C.c_int32, 12), ("s_enter", C.c_double, 16), ("s_leave", C.c_double, 24)]
PAIR = [("status", C.c_int32, 0), ("n_times", C.c_int32, 4), ("n_conflict", C.c_int32, 8), ("reserved", C.c_int32, 12), ("t_first", C.c_double, 16), ("s_first", C.c_double * 2, 24),
        ("min_separation", C.c_double, 40), ("t_min", C.c_double, 48), ("s_min", C.c_double * 2, 56), ("reserved1", C.c_double, 72)]
# the figures of the build DESIGN.md 4.10 records (tools/kernel_resources.py), as upper bounds: (VGPRs, scratch bytes per lane)
RECORDED = {"k_trajectory_tickets": (149, 168), "k_conflict_pairs": (52, 0)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import ConflictParams, ConflictResult, TrajectoryResult
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_conflict_params\s*\{\s*double\s+t_from\s*,\s*t_to\s*;\s*double\s+dt\s*;\s*double\s+margin\s*;\s*int32_t\s+hold_before\s*;\s*"
                     r"int32_t\s+hold_after\s*;\s*\}\s*pp_conflict_params\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_trajectory_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+n_present\s*;\s*int32_t\s+first\s*,\s*last\s*;\s*double\s+s_enter\s*,\s*s_leave\s*;"
                     r"\s*\}\s*pp_trajectory_result\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_conflict_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+n_times\s*;\s*int32_t\s+n_conflict\s*;\s*int32_t\s+reserved\s*;\s*double\s+t_first\s*;"
                     r"\s*double\s+s_first\[2\]\s*;\s*double\s+min_separation\s*;\s*double\s+t_min\s*;\s*double\s+s_min\[2\]\s*;\s*double\s+reserved1\s*;\s*\}\s*pp_conflict_result\s*;", txt)
    tail = (r"\s*int32_t\s+n_pairs\s*,\s*const\s+int32_t\s*\*\s*pairs\s*,\s*const\s+pp_conflict_params\s*\*\s*params\s*,\s*double\s*\*\s*poses_host\s*,"
            r"\s*pp_trajectory_result\s*\*\s*plans_host\s*,\s*pp_conflict_result\s*\*\s*results_host\s*\)\s*;")
    assert re.search(r"\bint\s+pp_pipeline_conflicts\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    assert re.search(r"\bint\s+pp_planner_conflicts\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*int32_t\s+n_queries\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_conflicts") and hasattr(lib, "pp_planner_conflicts")
    # the ctypes records are the C ones, field for field and offset for offset
    for cls, fields, size in ((ConflictParams, PARAMS, 40), (TrajectoryResult, PLAN, 32), (ConflictResult, PAIR, 80)):
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields]
        for n, t, off in fields:
            assert dict(cls._fields_)[n] is t or dict(cls._fields_)[n]._length_ == t._length_, n
            assert getattr(cls, n).offset == off, (cls.__name__, n)
        assert C.sizeof(cls) == size
    # ... and the library's own view of the sizes
    planner = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_conflicts.hpp")).read()
    for name, size in (("pp_conflict_params", 40), ("pp_trajectory_result", 32), ("pp_conflict_result", 80)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in planner


def test_both_kernels_are_built_as_one_wave_within_the_recorded_figures():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, (vgprs, scratch) in RECORDED.items():
        assert name in res, sorted(res)
        k = res[name]
        assert k["scratch_bytes_per_lane"] <= scratch <= reserve, k
        assert k["vgpr"] <= vgprs, k
        assert k["max_flat_workgroup_size"] == 64, k
        assert k["vgpr_spill"] == 0 and k["lds_bytes"] == 0, k  # (the trajectory kernel's LDS is dynamic: 16 B per path-capacity entry)
        assert name in design and "%d VGPRs" % vgprs in design and "%d B" % scratch in design
    assert '#include "pp_conflicts.hpp"' in src and '#include "pp_conflict_rule.hpp"' in src
    assert src.index('#include "pp_speed_profile.hpp"') < src.index('#include "pp_conflicts.hpp"')
    warm = src[src.index("hipError_t warm_up_held_kernels"):src.index("int warm_up_kernels")]
    assert "launch_trajectory(s, p->args" in warm and "launch_conflict_pairs(s, " in warm  # (their scratch is allocated at creation)
    held = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_held_plans.hpp")).read()
    assert "struct ConflictGroup" in held and src.count("held_grow(h, g.") >= 3


def test_the_kernels_text_leaves_the_arithmetic_to_the_rule():
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_conflicts.hpp")).read()
    for name in ("ppc::lattice_time", "ppc::position", "ppc::separation", "ppc::in_conflict", "ppc::closer", "ppc::earlier", "ppc::pair_of", "ppl::edge_of", "ppl::ratio_of",
                 "load_edge(", ".interpolate(", "disc_centre(", "__shfl_xor"):
        assert name in kernel, name
    assert "sqrt" not in kernel and "atomic" not in kernel.lower() and "asm" not in kernel
    rule = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_conflict_rule.hpp")).read()
    assert "ppv::step_time" in rule and "__builtin_sqrt" in rule and "__builtin_ceil" in rule and "__builtin_floor" in rule
    assert not re.search(r"\b(sin|cos|exp|log|pow|hypot|fmin|fmax|sqrt)\s*\(", rule)
    assert "PPC_INLINE" in rule and "__host__ __device__" in rule


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.conflicts)
    assert list(sig.parameters) == ["self", "tickets", "t_start", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "poses"]
    assert [sig.parameters[k].default for k in ("pairs", "t_from", "dt", "margin", "hold_before", "hold_after", "poses")] == [None, 0.0, 0.1, 0.0, False, False, False]
    sig = inspect.signature(planner.HybridAStarBatch.conflicts)
    assert list(sig.parameters) == ["self", "t_start", "n_queries", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "poses"]
    assert planner.conflict_lattice(0.0, 60.0, 0.1) == (0, 601) and planner.conflict_lattice(-1.05, 1.05, 0.1) == (-10, 21) and planner.conflict_lattice(0.55, 0.55, 0.25)[1] == 0


def test_pyplanning_binds_conflicts():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.conflicts)
    doc = nav.HybridAStarPipeline.conflicts.__doc__
    assert all(w in doc for w in ["tickets", "t_start", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "poses", "speed_profile"])


def test_the_cpp_mirror_test_program_compiles():
    """tests/cpp/test_pipeline_conflicts.cpp (run by the GPU suite) builds against the C++ mirror: Conflicts and its records exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_conflicts_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"Conflicted\s+Conflicts\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*const\s+std::vector<double>&\s*tStart\s*,", hpp)
