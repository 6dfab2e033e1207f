"""CPU-side gate on the SCALAR spills of the rows kernels' expansion loop (no GPU needed; the listing is built the way
tests/test_kernel_resources.py builds it and attributed to the phases between the kernel's own ROWS_STAMP markers by tools/isa_spill_map.py).

A wave has about a hundred SGPRs.  Read as members of the by-value kernel arguments, the map's bounds, origins, resolutions and reciprocals, the
heuristic's table geometry, the lattice and the key space are loop invariants: the compiler loaded them all in front of the loop and kept what
did not fit in lanes of spill VGPRs -- `.sgpr_spill_count` 464, and 1 152 v_readlane + 156 v_writelane in the five per-expansion phases of
k_hybrid_search_rows<true> (6 602 instructions: one in five a spill reload or save, each a VALU issue slot on a SIMD that two tile waves also
issue from).  The loop now reads them from the kernel-argument segment in scalar loads that cannot leave it (pp_rows_rs.hpp:
rows_kernargs_here; DESIGN.md section 4.4, "scalar spills"; profiles/search_scalar_spills.txt).  The row primitives use ds_bpermute and DPP,
not lane reads, so lane reads + writes count the spill traffic.

Gates: the finished build's figure plus 5 % for compiler noise, each below half of its own parent's figure."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ("pop+refill", "node", "children", "insertion", "node-records")
BODY = "pp_planner_rows.hpp"

# kernel (as its mangled name spells it) -> (parent's lane reads + writes in the per-expansion phases, this build's, gate)
KERNELS = {
    "k_hybrid_search_rowsILb1E": (1_308, 352, 369),            # pipeline form: the bench's steady state
    "k_hybrid_search_rows_footprintILb1E": (2_075, 486, 510),  # pipeline form with a vehicle footprint (the footprint is read from the segment too)
}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from pathplanning_amd import build
    csrc = os.path.join(ROOT, "pathplanning_amd", "csrc")
    path = str(tmp_path_factory.mktemp("scalar_spills") / "planner.s")
    flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
    subprocess.check_call([build.hipcc()] + flags + ["-gline-tables-only", "-S", "--cuda-device-only", "-o", path, os.path.join(csrc, "pp_planner.hip")],
                          stderr=subprocess.DEVNULL)
    return path


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_spilled_scalars_stay_out_of_the_expansion_loop(listing, kernel):
    import isa_spill_map
    phases = isa_spill_map.phases_from_stamps(os.path.join(ROOT, "pathplanning_amd", "csrc", BODY))
    m = isa_spill_map.lane_map(listing, kernel, BODY, phases)
    assert all(m[p][0] > 0 for p in HOT), m  # (the attribution found the phases)
    reads, writes = sum(m[p][1] for p in HOT), sum(m[p][2] for p in HOT)
    parent, _, gate = KERNELS[kernel]
    print(kernel, "per-expansion phases:", sum(m[p][0] for p in HOT), "instructions,", reads, "lane reads +", writes, "lane writes; gate", gate, "; parent", parent)
    assert 2 * gate <= parent  # the aim: at most half of the parent's
    assert reads + writes <= gate, (kernel, reads, writes, gate, m)
    assert sum(m[p][4] for p in HOT) > 0, m  # the constants do come in scalar loads inside the loop
