"""CPU side of the streaming pipeline's footprint (pp_pipeline_set_footprint, k_hybrid_search_rows_footprint<true>): the entry is declared and
exported, the kernel is in the built code object with its scratch and spill figures at the values DESIGN.md section 4.8b records, and its
scratch traffic in the per-expansion phases is where tools/isa_spill_map.py measured it (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "k_hybrid_search_rows_footprint<true>"
# what the compiler produces for the finished kernel, as ceilings (k_hybrid_search_rows<true>, the same text without the footprint: 528 B / 113)
MAX_SCRATCH_BYTES, MAX_VGPR_SPILLS = 600, 149
# scratch loads / stores in the per-expansion phases (k_hybrid_search_rows<true>: 23 / 1); the growth sits in the children phase, whose march
# and pose checks loop over the discs
MAX_HOT_LOADS, MAX_HOT_STORES = 62, 7
HOT = ("pop+refill", "node", "children", "insertion", "node-records")


def test_the_entry_is_declared_and_exported():
    from pathplanning_amd import build
    txt = open(os.path.join(ROOT, "include", "pp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+pp_pipeline_set_footprint\s*\(\s*pp_pipeline\s*\*\s*\w+\s*,\s*pp_footprint\s*\*\s*\w+\s*\)\s*;", txt)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "pp_pipeline_set_footprint")
    from pathplanning_amd import planner
    assert callable(planner.HybridAStarPipeline.set_footprint) and isinstance(planner.HybridAStarPipeline.footprint, property)


def test_the_footprint_rows_kernel_is_built_within_its_figures():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    assert KERNEL in res, sorted(res)
    k = res[KERNEL]
    assert k["scratch_bytes_per_lane"] <= MAX_SCRATCH_BYTES and k["vgpr_spill"] <= MAX_VGPR_SPILLS, k
    # the pipeline form only: the batch rows planner takes no footprint
    assert "k_hybrid_search_rows_footprint<false>" not in res
    # the point kernels are separate kernels under their own names
    assert "k_hybrid_search_rows<true>" in res and "k_hybrid_search_rows<false>" in res


def test_the_footprint_rows_kernel_keeps_scratch_traffic_out_of_the_expansion_path(tmp_path):
    import isa_spill_map
    from pathplanning_amd import build
    csrc = os.path.join(ROOT, "pathplanning_amd", "csrc")
    listing = str(tmp_path / "planner.s")
    flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
    subprocess.check_call([build.hipcc()] + flags + ["-gline-tables-only", "-S", "--cuda-device-only", "-o", listing, os.path.join(csrc, "pp_planner.hip")],
                          stderr=subprocess.DEVNULL)
    phases = isa_spill_map.phases_from_stamps(os.path.join(csrc, "pp_planner_rows.hpp"))
    m = isa_spill_map.spill_map(listing, "k_hybrid_search_rows_footprintILb1E", "pp_planner_rows.hpp", phases)
    assert all(m[p][0] > 0 for p in HOT if p != "node-records"), m  # (the attribution found the phases)
    loads, stores = sum(m[p][1] for p in HOT), sum(m[p][2] for p in HOT)
    print("per-expansion phases of %s: %d scratch loads, %d stores; %s" % (KERNEL, loads, stores, {p: m[p] for p in HOT}))
    assert loads <= MAX_HOT_LOADS and stores <= MAX_HOT_STORES, m
    assert m["reeds-shepp"][1] > loads  # the spills live where they cost least
