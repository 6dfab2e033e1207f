"""CPU side of speed profiles along held plans (pp_pipeline_speed_profile / pp_planner_speed_profile, k_speed_profile_tickets in
pathplanning_amd/csrc/pp_speed_profile.hpp): the entries and the records are declared and exported, the kernel is in the built code object as one
wave per workgroup within the resource figures DESIGN.md 4.10 records, and the Python layers, the C++ mirror and the pybind11 module expose the call
(no GPU needed)."""
import ctypes as C
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PARAMS = ["spacing", "v_max_forward", "v_max_reverse", "a_acc", "a_dec", "a_lat", "dwell", "clearance_gain", "v_floor"]
FIELDS = [("status", C.c_int32, 0), ("n_samples", C.c_int32, 4), ("n_cusps", C.c_int32, 8), ("reserved", C.c_int32, 12), ("length", C.c_double, 16), ("s_first", C.c_double, 24),
          ("s_last", C.c_double, 32), ("duration", C.c_double, 40), ("v_peak", C.c_double, 48), ("min_clearance", C.c_double, 56), ("s_min_clearance", C.c_double, 64)]
# the figures of the build DESIGN.md 4.10 records (tools/kernel_resources.py), as upper bounds
MAX_VGPRS, MAX_SCRATCH_BYTES_PER_LANE = 198, 168


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pp_hip.h")).read(), flags=re.S)


def test_the_entries_and_the_records_are_declared_and_exported():
    from pathplanning_amd import build
    from pathplanning_amd._lib import SpeedProfileParams, SpeedProfileResult
    txt = _header()
    assert re.search(r"typedef\s+struct\s+pp_speed_profile_params\s*\{\s*" + r"\s*".join(r"double\s+%s\s*;" % n for n in PARAMS) + r"\s*\}\s*pp_speed_profile_params\s*;", txt)
    members = [r"int32_t\s+%s\s*;" % n for n, t, _ in FIELDS if t is C.c_int32] + [r"double\s+length\s*;", r"double\s+s_first\s*,\s*s_last\s*;"] + \
              [r"double\s+%s\s*;" % n for n in ("duration", "v_peak", "min_clearance", "s_min_clearance")]
    assert re.search(r"typedef\s+struct\s+pp_speed_profile_result\s*\{\s*" + r"\s*".join(members) + r"\s*\}\s*pp_speed_profile_result\s*;", txt)
    tail = (r"\s*const\s+double\s*\*\s*from_length\s*,\s*const\s+double\s*\*\s*to_length\s*,\s*const\s+double\s*\*\s*v_start\s*,\s*const\s+double\s*\*\s*v_end\s*,"
            r"\s*const\s+pp_speed_profile_params\s*\*\s*params\s*,\s*int32_t\s+max_samples\s*,\s*double\s*\*\s*samples_host\s*,\s*pp_speed_profile_result\s*\*\s*results_host\s*\)\s*;")
    assert re.search(r"\bint\s+pp_pipeline_speed_profile\s*\(\s*pp_pipeline\s*\*\s*\w*\s*,\s*pp_map\s*\*\s*target\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*," + tail, txt)
    assert re.search(r"\bint\s+pp_planner_speed_profile\s*\(\s*pp_planner\s*\*\s*\w*\s*,\s*pp_map\s*\*\s*target\s*,\s*int32_t\s+n_queries\s*," + tail, txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_speed_profile") and hasattr(lib, "pp_planner_speed_profile")
    # the ctypes records are the C ones
    assert [(n, t) for n, t in SpeedProfileParams._fields_] == [(n, C.c_double) for n in PARAMS] and C.sizeof(SpeedProfileParams) == 72
    assert [n for n, _ in SpeedProfileResult._fields_] == [n for n, _, _ in FIELDS]
    for n, t, off in FIELDS:
        assert dict(SpeedProfileResult._fields_)[n] is t and getattr(SpeedProfileResult, n).offset == off, n
    assert C.sizeof(SpeedProfileResult) == 72


def test_the_kernel_is_built_as_one_wave_within_the_recorded_figures():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    assert "k_speed_profile_tickets" in res, sorted(res)
    k = res["k_speed_profile_tickets"]
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    assert k["scratch_bytes_per_lane"] <= MAX_SCRATCH_BYTES_PER_LANE <= reserve, k
    assert k["vgpr"] <= MAX_VGPRS, k
    assert k["max_flat_workgroup_size"] == 64, k
    assert k["vgpr_spill"] == 0 and k["lds_bytes"] == 0, k  # (its LDS is dynamic: 20 B per path-capacity entry)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_speed_profile_tickets" in design and "%d VGPRs" % MAX_VGPRS in design and "%d B" % MAX_SCRATCH_BYTES_PER_LANE in design
    assert '#include "pp_speed_profile.hpp"' in src and '#include "pp_speed_rule.hpp"' in src
    assert src.index('#include "pp_locate.hpp"') < src.index('#include "pp_speed_profile.hpp"')
    assert "launch_speed_profile(s, p->args" in src[src.index("hipError_t warm_up_held_kernels"):src.index("int warm_up_kernels")]  # (its scratch is allocated at creation)
    # the kernel and the host program share the rule: the kernel's text has no cap, envelope or step arithmetic of its own
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_speed_profile.hpp")).read()
    for name in ("ppv::cap(", "ppv::cap_squared", "ppv::is_cusp", "ppv::forward_key", "ppv::forward_limit", "ppv::backward_key", "ppv::backward_limit", "ppv::envelope", "ppv::speed(",
                 "ppv::step_time", "ppv::lower_clearance", "pps::edge_steps", "pps::sample_ratio", "pps::sample_arc_length", "pps::in_window", "E.curvature(ratio)", "E.direction(ratio)"):
        assert name in kernel, name
    assert "sqrt" not in kernel and "atomic" not in kernel.lower() and "asm" not in kernel
    rule = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_speed_rule.hpp")).read()
    assert "__builtin_sqrt" in rule and not re.search(r"\b(sin|cos|exp|log|pow|hypot|fmin|fmax)\s*\(", rule)
    # the Reeds-Shepp curvature is read from the motion direction() selects: one selection, two accessors
    rs = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_rs_device.hpp")).read()
    assert rs.count("int motion_at(double ratio) const") == 1 and rs.count("const int i = motion_at(ratio);") == 2


def test_the_python_wrappers_have_the_calls():
    from pathplanning_amd import planner
    sig = inspect.signature(planner.HybridAStarPipeline.speed_profile)
    assert list(sig.parameters) == ["self", "tickets", "map_set", "from_length", "to_length", "v_start", "v_end", "max_samples", "samples", "limits"]
    assert [sig.parameters[k].default for k in ("map_set", "from_length", "to_length", "v_start", "v_end", "max_samples", "samples")] == [None, None, None, None, None, 2048, True]
    sig = inspect.signature(planner.HybridAStarBatch.speed_profile)
    assert list(sig.parameters) == ["self", "n_queries", "map_set", "from_length", "to_length", "v_start", "v_end", "max_samples", "samples", "limits"]
    assert sorted(planner.SPEED_PROFILE_DEFAULTS) == sorted(PARAMS)


def test_pyplanning_binds_speed_profile():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert callable(nav.HybridAStarPipeline.speed_profile)
    doc = nav.HybridAStarPipeline.speed_profile.__doc__
    assert all(w in doc for w in PARAMS + ["tickets", "max_samples", "from_length", "to_length", "v_start", "v_end", "validator"])


def test_the_cpp_mirror_test_program_compiles():
    """tests/cpp/test_pipeline_speed_profile.cpp (run by the GPU suite) builds against the C++ mirror: SpeedProfile and its records exist there"""
    from pathplanning_amd import build
    exe = build.build_pipeline_speed_profile_test(verbose=False)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "pathplanning_amd", "host", "planner_hip.hpp")).read()
    assert re.search(r"std::vector<SpeedProfiled>\s+SpeedProfile\s*\(\s*const\s+std::vector<uint64_t>&\s*tickets\s*,\s*double\s+spacing\s*,\s*const\s+SpeedLimits&\s*limits\s*,", hpp)
