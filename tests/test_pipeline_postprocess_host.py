"""CPU side of the pipeline's post-processing by ticket (pp_pipeline_postprocess / pp_pipeline_get_processed_paths, k_postprocess_tickets): the
entries are declared and exported, the second form of the post-processing kernel is in the built code object within the planner's
headroom, the first form kept its figures, and the Python layers expose the calls (no GPU needed)."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# k_postprocess as the commit before k_postprocess_tickets built it (tools/kernel_resources.py): 225 VGPRs, 106 SGPRs, 40 B of LDS and ...
PARENT_SCRATCH_BYTES, PARENT_VGPR_SPILLS, PARENT_SGPR_SPILLS = 720, 0, 47


def _resources():
    from pathplanning_amd import build
    import kernel_resources
    return {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}


def test_the_entries_are_declared_and_exported():
    from pathplanning_amd import build
    txt = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    assert "-2: a smoothed sample fails the vehicle footprint" in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+pp_pipeline_postprocess\s*\(\s*pp_pipeline\s*\*\s*\w+\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,\s*float\s+path_interpolation\s*,"
                     r"\s*const\s+pp_smoother_params\s*\*\s*smoother\s*,\s*int32_t\s+max_points\s*,\s*pp_post_result\s*\*\s*results_host\s*\)\s*;", txt)
    assert re.search(r"\bint\s+pp_pipeline_get_processed_paths\s*\(\s*pp_pipeline\s*\*\s*\w+\s*,\s*int32_t\s+n\s*,\s*const\s+uint64_t\s*\*\s*tickets\s*,\s*int32_t\s+max_points\s*,"
                     r"\s*double\s*\*\s*sampled_host\s*,\s*uint8_t\s*\*\s*cusp_host\s*,\s*double\s*\*\s*smoothed_host\s*,\s*int32_t\s*\*\s*n_points_host\s*,\s*int32_t\s+release\s*\)\s*;", txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_postprocess") and hasattr(lib, "pp_pipeline_get_processed_paths")


def test_the_ticket_form_of_the_kernel_is_built_within_the_planner_headroom():
    res = _resources()
    assert "k_postprocess_tickets" in res, sorted(res)
    k = res["k_postprocess_tickets"]
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    assert k["vgpr"] <= 256 and k["scratch_bytes_per_lane"] <= reserve, k
    assert k["max_flat_workgroup_size"] == 256


def test_the_batch_form_of_the_kernel_kept_its_figures():
    k = _resources()["k_postprocess"]
    assert k["scratch_bytes_per_lane"] <= PARENT_SCRATCH_BYTES and k["vgpr_spill"] <= PARENT_VGPR_SPILLS and k["sgpr_spill"] <= PARENT_SGPR_SPILLS, k


def test_the_python_wrapper_has_the_calls():
    from pathplanning_amd import planner
    P = planner.HybridAStarPipeline
    assert callable(P.postprocess) and callable(P.get_processed_paths)
    assert "postprocess(tickets)" in P.postprocess_held.__doc__  # the old call points to the new one
    import inspect
    assert list(inspect.signature(P.postprocess).parameters) == ["self", "tickets", "path_interpolation", "smoother", "max_points"]
    assert list(inspect.signature(P.get_processed_paths).parameters) == ["self", "tickets", "release"]


def test_pyplanning_binds_the_pipeline():
    import importlib
    from pathplanning_amd import build
    build.build_pyplanning(verbose=False)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "lib"))
    nav = importlib.import_module("pyplanning")
    assert hasattr(nav, "HybridAStarPipeline")
    for name in ("initialize", "submit", "poll", "post_process", "get_path", "get_graph_search_path", "release", "in_flight", "free_slots", "set_heuristic_clearance"):
        assert callable(getattr(nav.HybridAStarPipeline, name)), name
    assert nav.SmoothingStatus.COLLISION.value == -2
    pipe = nav.HybridAStarPipeline(nav.HybridAStarSearchParameters(), capacity=16, max_nodes=32768, search_rows=8)  # (no device work before initialize)
    assert pipe.in_flight() == 0 and pipe.free_slots() == 0 and pipe.poll() == []
