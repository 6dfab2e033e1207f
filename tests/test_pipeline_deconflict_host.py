"""CPU side of start delays that clear conflicts between held plans (pp_pipeline_deconflict / pp_planner_deconflict, k_delay_level in
pathplanning_amd/csrc/pp_deconflict.hpp): the entries and both records are declared, exported and mirrored in ctypes offset for offset, the kernel is
in the built code object as one wave per workgroup within the resource figures DESIGN.md 4.10 records, its text leaves the rule to
pp_delay_rule.hpp and uses neither atomics nor assembly, and the Python layers, the C++ mirror and the pybind11 module expose the call (no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LATTICE = [("t_from", C.c_double, 0), ("t_to", C.c_double, 8), ("dt", C.c_double, 16), ("margin", C.c_double, 24), ("hold_before", C.c_int32, 32), ("hold_after", C.c_int32, 36)]
RESULT = [("status", C.c_int32, 0), ("delay_steps", C.c_int32, 4), ("n_tried", C.c_int32, 8), ("blocker", C.c_int32, 12), ("t_start", C.c_double, 16), ("t_block", C.c_double, 24),
          ("s_block", C.c_double * 2, 32)]
# the figures of the build DESIGN.md 4.10 records (tools/kernel_resources.py), as upper bounds
RECORDED = dict(vgpr=58, sgpr=96, scratch=0, lds=0)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import ConflictParams, DelayParams, DelayResult
    from pathplanning_amd.planner import DELAY_DTYPE
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_delay_params\s*\{\s*pp_conflict_params\s+lattice\s*;\s*int32_t\s+max_delay_steps\s*;\s*int32_t\s+reserved\s*;\s*\}\s*pp_delay_params\s*;", txt)
    assert re.search(r"typedef\s+struct\s+pp_delay_result\s*\{\s*int32_t\s+status\s*;\s*int32_t\s+delay_steps\s*;\s*int32_t\s+n_tried\s*;\s*int32_t\s+blocker\s*;\s*double\s+t_start\s*;"
                     r"\s*double\s+t_block\s*;\s*double\s+s_block\[2\]\s*;\s*\}\s*pp_delay_result\s*;", txt)
    tail = r"\s*int32_t\s+n_pairs\s*,\s*const\s+int32_t\s*\*\s*pairs\s*,\s*const\s+pp_delay_params\s*\*\s*params\s*,\s*pp_delay_result\s*\*\s*results_host\s*\)\s*;"
    assert re.search(r"\bint\s+pp_pipeline_deconflict\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    assert re.search(r"\bint\s+pp_planner_deconflict\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*int32_t\s+n_queries\s*,\s*const\s+double\s*\*\s*t_start\s*," + tail, txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_deconflict") and hasattr(lib, "pp_planner_deconflict")
    # the ctypes records are the C ones, field for field and offset for offset
    assert [n for n, _ in DelayParams._fields_] == ["lattice", "max_delay_steps", "reserved"] and dict(DelayParams._fields_)["lattice"] is ConflictParams
    assert (DelayParams.lattice.offset, DelayParams.max_delay_steps.offset, DelayParams.reserved.offset) == (0, 40, 44)
    assert dict(DelayParams._fields_)["max_delay_steps"] is C.c_int32 and dict(DelayParams._fields_)["reserved"] is C.c_int32
    for n, t, off in LATTICE:
        assert dict(ConflictParams._fields_)[n] is t and getattr(ConflictParams, n).offset == off
    assert [n for n, _ in DelayResult._fields_] == [n for n, _, _ in RESULT]
    for n, t, off in RESULT:
        assert dict(DelayResult._fields_)[n] is t or dict(DelayResult._fields_)[n]._length_ == t._length_, n
        assert getattr(DelayResult, n).offset == off, n
    assert C.sizeof(DelayParams) == 48 and C.sizeof(DelayResult) == 48
    # ... the numpy record the wrappers return is the same record
    assert DELAY_DTYPE.itemsize == 48 and [(n, DELAY_DTYPE.fields[n][1]) for n in DELAY_DTYPE.names] == [(n, off) for n, _, off in RESULT]
    assert DELAY_DTYPE["s_block"].shape == (2,) and DELAY_DTYPE["t_start"] == np.float64 and DELAY_DTYPE["blocker"] == np.int32
    # ... and the library's own view of the sizes
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_deconflict.hpp")).read()
    for name in ("pp_delay_params", "pp_delay_result"):
        assert "static_assert(sizeof(%s) == 48" % name in kernel


def test_the_kernel_is_built_as_one_wave_within_the_recorded_figures():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_delay_level" in res, sorted(res)
    k = res["k_delay_level"]
    assert k["max_flat_workgroup_size"] == 64, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["scratch_bytes_per_lane"] <= RECORDED["scratch"] <= reserve, k
    assert k["vgpr"] <= RECORDED["vgpr"] and k["sgpr"] <= RECORDED["sgpr"] and k["lds_bytes"] <= RECORDED["lds"], k
    assert "k_delay_level" in design and "%d VGPRs" % RECORDED["vgpr"] in design and "%d SGPRs" % RECORDED["sgpr"] in design
    assert '#include "pp_deconflict.hpp"' in src and '#include "pp_delay_rule.hpp"' in src
    assert src.index('#include "pp_conflicts.hpp"') < src.index('#include "pp_deconflict.hpp"')
    warm = src[src.index("hipError_t warm_up_held_kernels"):src.index("int warm_up_kernels")]
    assert "launch_delay_level(s, " in warm  # (a failure to set the kernel up is an error code at creation)
    held = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_held_plans.hpp")).read()
    assert "struct DelayGroup" in held and "held_grow(h, g.vehicles" in src and "held_grow(h, c.doubles" in src


def test_the_kernels_text_leaves_the_rule_to_the_rule_and_synchronises_by_stream_order_alone():
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_deconflict.hpp")).read()
    for name in ("ppy::column", "ppy::key", "ppy::before", "ppy::kNoKey", "ppy::time_of", "ppy::partner_of", "ppc::separation", "ppc::in_conflict", "ppc::lattice_time",
                 "disc_centre(", "__shfl_xor", "__launch_bounds__(kDelayLanes)"):
        assert name in kernel, name
    code = re.sub(r"//.*", "", kernel)
    assert "sqrt" not in code and "atomic" not in kernel.lower() and "asm" not in kernel and "__syncthreads" not in code and "while" not in code
    assert "k_trajectory_tickets" not in code and "k_conflict_pairs" not in code  # (it launches neither: the host does, unchanged)
    rule = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_delay_rule.hpp")).read()
    assert "PPY_INLINE" in rule and "__host__ __device__" in rule
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", rule)
    assert includes == ["cstddef", "cstdint", "pp_conflict_rule.hpp"]  # no library function
    assert not re.search(r"\b(std::|malloc|new |memcpy|memset|sort)\b", re.sub(r"//.*", "", rule))
    for name in ("column(", "key(", "before(", "partner_offsets(", "partner_list(", "levels(", "members_by_level("):
        assert name in rule, name
    # the conflict kernels' file is as it was: the delay kernel lives in its own
    assert "k_delay_level" not in open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_conflicts.hpp")).read()


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.deconflict)
    assert list(sig.parameters) == ["self", "tickets", "t_start", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "max_delay_steps"]
    assert [sig.parameters[k].default for k in ("pairs", "t_from", "dt", "margin", "hold_before", "hold_after", "max_delay_steps")] == [None, 0.0, 0.1, 0.0, False, False, 0]
    assert sig.parameters["t_to"].default == inspect.signature(planner.HybridAStarPipeline.conflicts).parameters["t_to"].default
    sig = inspect.signature(planner.HybridAStarBatch.deconflict)
    assert list(sig.parameters) == ["self", "t_start", "n_queries", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "max_delay_steps"]
    assert list(planner.delay_levels(0, [])) == [] and list(planner.delay_levels(4, None)) == [0, 1, 2, 3] and list(planner.delay_levels(4, [])) == [0, 0, 0, 0]
    assert list(planner.delay_levels(5, [(3, 0), (0, 1), (4, 3), (1, 0)])) == [0, 1, 0, 1, 2]
    assert planner.delay_levels(3, None).dtype == np.int32


def test_pyplanning_binds_deconflict():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.deconflict)
    doc = nav.HybridAStarPipeline.deconflict.__doc__
    assert all(w in doc for w in ["tickets", "t_start", "pairs", "t_from", "t_to", "dt", "margin", "hold_before", "hold_after", "max_delay_steps", "speed_profile"])


def test_the_cpp_mirror_test_program_compiles():
    """tests/cpp/test_pipeline_deconflict.cpp (run by the GPU suite) builds against the C++ mirror: Deconflict and its record exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_deconflict_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"std::vector<Delay>\s+Deconflict\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*const\s+std::vector<double>&\s*tStart\s*,", hpp)
